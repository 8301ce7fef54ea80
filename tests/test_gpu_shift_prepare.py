"""GPU: a prepared weight side for forward-only shift-ADC layers (cimq_module_prepare_shift) and shift-ADC networks
as one cimq_net_forward plan.

Every comparison is between two runs of this library and is on bit patterns: the call with the prepared weight side
(``Conv2dLSQCiM.forward`` / ``forward_fused`` under no-grad, which keep ``_inf_prep``) against the same call with
``wprep=None`` through ``cim_module_conv_epilogue`` / ``cim_module_conv_codes`` -- the parent's only path.  A
forward-only shift layer whose activations have four or fewer slices also quantises its input in the forward
kernel's row staging (Route::actq), so with the prepared side it is one launch: the kernel-count test pins that.

Shapes: B = 2 throughout, the smallest the fused shift path takes (M = B * P must be a multiple of 128)."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from slice_cases import SHIFT_CASES
from test_epilogue_host import randomise_bn
from test_gpu_net import _bits, _head_bars, _logit_bar, _loop_last_plane
from test_gpu_shift_fullbatch import _build
from test_inference_host import INF

pytestmark = pytest.mark.gpu


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


# ---------------------------------------------------------------------------------------------------
# the layers
# ---------------------------------------------------------------------------------------------------
_S6 = next(c for c, ok in SHIFT_CASES if ok == 1 and c["xbar"] == 64)  # 2-bit slices: the run-time word table
#       C,  O,  H, stride, bits, xbar, slice width, signed input
LAYERS = {
    "w2a2_16": (16, 16, 8, 1, 2, 64, 1, False),    # one m-tile; K = 144: three tiles, the last of 16 rows
    "w2a2_s2": (16, 32, 16, 2, 2, 64, 1, False),
    "w2a2_64": (64, 64, 8, 1, 2, 64, 1, False),    # nine tiles
    "w3a3_x128": (16, 16, 8, 1, 3, 128, 1, False),  # test_inference_host's ``shift`` case
    "w8a8_first": (3, 16, 16, 1, 8, 64, 1, True),   # NBP 8: prepared, not staged (two launches)
    "slices2": (_S6["C"], _S6["O"], _S6["H"], _S6["s"][0], _S6["wb"], _S6["xbar"], _S6["wbs"], False),
}
_BUILT = {}


def _beta(m, seed):
    """beta uniform in +-0.3 alpha, every entry non-zero"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(m.alpha_cim.shape, generator=g) * 2 - 1
    u = torch.where(u.abs() < 0.05, torch.full_like(u, 0.05) * torch.where(u < 0, -1.0, 1.0), u)
    assert bool((u.abs() >= 0.05).all())
    a = m.alpha_cim.detach()
    b = (0.3 * u).to(a.device) * a
    assert bool(((b != 0) == (a != 0)).all()) and bool((a != 0).any()) and bool((b.abs() <= 0.3 * a.abs()).all())
    return b


def _layer(name, dev):
    """(module in its steady state, x): alpha_cim spread as test_gpu_shift_fullbatch spreads it, beta as above,
    x = relu(randn) (signed for the first conv).  Built once per case."""
    if name not in _BUILT:
        C, O, H, s, bits, xbar, bs, signed = LAYERS[name]
        seed = 9700 + sum(map(ord, name))
        m, _, x, *_ = _build(dev, C, O, H, s, bits, 2, seed, signed, xbar=xbar, bs=bs)
        with torch.no_grad():
            m.beta_cim.copy_(_beta(m, seed + 1))
        _BUILT[name] = (m, torch.from_numpy(x).to(dev))
    return _BUILT[name]


def _supported(m, x):
    F, L = _F(), _L()
    desc, _ = F._shift_module_descs(tuple(x.shape), m.weight, m.stride, m.padding, m.dilation, m.nbits_a, m.abitslice,
                                    m.nbits_w, m.wbitslice, m.xbar, m.nbits_alpha)
    desc.options = INF
    return L.load().cimq_module_shift_supported(ctypes.byref(desc))


def _args(m):
    return (m.weight, m.alpha_act, m.alpha_weight, m.alpha_cim, m.binary_mask, m.signed_act, m.stride, m.padding,
            m.dilation, m.nbits_a, m.abitslice, m.nbits_w, m.wbitslice, m.adcbits, m.xbar, m.nbits_alpha)


def _unprepared(m, x, scale, shift, beta=None, **kw):
    """the call as the parent makes it: no prepared weight side"""
    F = _F()
    fn = F.cim_module_conv_codes if (x.dtype == torch.uint8 or "out_quant" in kw) else F.cim_module_conv_epilogue
    with torch.no_grad():
        return fn(x, *_args(m), scale, shift, beta_cim=m.beta_cim if beta is None else beta, wprep=None, **kw)


def _prepared(m, x, scale, shift, **kw):
    try:
        m.eval()
        with torch.no_grad():
            y = m.forward_fused(x, scale, shift, **kw)
        assert m._inf_prep is not None  # the weight side was prepared and kept
        return y
    finally:
        m.train()


def _tables(O, shape, seed, dev, std):
    g = torch.Generator().manual_seed(seed)
    scale = torch.randn(O, generator=g).to(dev)
    shift = (torch.randn(O, generator=g) * std).to(dev)
    res = (torch.randn(shape, generator=g) * std).to(dev)
    return scale, shift, res


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == torch.float32:
        assert torch.equal(_bits(a), _bits(b)), (what, float((a - b).abs().max()))
    else:
        assert torch.equal(a, b), what


@pytest.mark.parametrize("name", list(LAYERS))
def test_prepared_equals_unprepared(cuda_device, monkeypatch, name):
    F, L = _F(), _L()
    m, x = _layer(name, cuda_device)
    assert _supported(m, x) == 1 and m._shift_fused(x)
    O = m.out_channels
    one, zero = torch.ones(O, device=cuda_device), torch.zeros(O, device=cuda_device)
    # beta matters, on the unprepared call: a build blind to beta would pass everything below
    plain = _unprepared(m, x, one, zero)
    assert not torch.equal(plain, _unprepared(m, x, one, zero, beta=torch.zeros_like(m.beta_cim)))
    scale, shift, res = _tables(O, plain.shape, 50 + sum(map(ord, name)), cuda_device, float(plain.std()))
    # the prepared call hands the library a weight side, the direct one none
    seen = []
    lib = L.load()
    real = lib.cimq_module_forward_epilogue

    def spy(*a):
        seen.append(bool(a[1].wprep))
        return real(*a)
    monkeypatch.setattr(lib, "cimq_module_forward_epilogue", spy)
    got = _prepared(m, x, scale, shift, residual=res, relu=True)
    want = _unprepared(m, x, scale, shift, residual=res, relu=True)
    monkeypatch.undo()
    assert seen == [True, False]
    _same(got, want, "residual + relu")
    frac = float((want == 0).float().mean())
    assert 0.02 < frac < 0.98, frac  # (ReLU cuts, and not everything)
    _same(_prepared(m, x, scale, shift), _unprepared(m, x, scale, shift), "affine alone")
    # codes out (for a w2a2 consumer), with and without the fp32 plane
    cons = copy.deepcopy(_layer("w2a2_16", cuda_device)[0])
    with torch.no_grad():  # (the consumer's step size to the scale of what it is fed)
        cons.alpha_act.fill_(float(want[want > 0].mean()) / 2)
    oq = cons._code_quant(plain.numel())
    yf, q = _prepared(m, x, scale, shift, residual=res, relu=True, out_quant=cons)
    wf, wq = _unprepared(m, x, scale, shift, residual=res, relu=True, out_quant=oq)
    _same(yf, want, "out_quant: fp32")
    _same(yf, wf, "out_quant: fp32 against the unprepared call")
    _same(q, wq, "out_quant: codes")
    assert int(q.min()) == 0 and 2 <= int(q.max()) <= 3  # (the codes vary; 4 would be the NaN code)
    _same(_prepared(m, x, scale, shift, residual=res, relu=True, out_quant=cons, keep_float=False),
          _unprepared(m, x, scale, shift, residual=res, relu=True, out_quant=oq, keep_float=False), "codes alone")
    # codes in: every layer whose Qp + 1 fits a byte (not the 8-bit first conv: cimq_module_codes_supported)
    in_ok = m.codes_ready(x)[0]
    assert in_ok == (m.nbits_a < 8)
    if in_ok:
        xq = m.act_codes(x.cpu()).to(cuda_device)
        gq = _prepared(m, xq, scale, shift, residual=res, relu=True)
        _same(gq, _unprepared(m, xq, scale, shift, residual=res, relu=True), "uint8 input")
        _same(gq, want, "uint8 input against the fp32 input")
        yq, qq = _prepared(m, xq, scale, shift, residual=res, relu=True, out_quant=cons)
        _same(yq, want, "uint8 input, out_quant: fp32")
        _same(qq, wq, "uint8 input, out_quant: codes")
        _same(_prepared(m, xq, scale, shift, residual=res, relu=True, out_quant=cons, keep_float=False), wq,
              "uint8 input, codes alone")
    # forward under no-grad (prepared) against the same forward with grad enabled (the training kernels)
    try:
        m.eval()
        with torch.no_grad():
            inf = m(x)
        assert inf.grad_fn is None and m._inf_prep is not None
        trn = m(x.clone().requires_grad_(True)).detach()
    finally:
        m.train()
    _same(inf, trn, "forward: no-grad against grad enabled")
    _same(inf, plain, "forward against the identity epilogue")


def test_nonfinite_beta_travels_in_the_prepared_buffer(cuda_device):
    """one +inf entry of beta: the literal-ADC flag is part of the prepared buffer (the int32 at wprep_bytes - 512:
    ctx_layout puts flags and then the step sizes, 256 bytes each, last in the weight side), and the output is the
    unprepared call's bit for bit"""
    m0, x = _layer("w2a2_16", cuda_device)
    O = m0.out_channels
    one, zero = torch.ones(O, device=cuda_device), torch.zeros(O, device=cuda_device)
    flags = {}
    outs = {}
    for key in ("finite", "inf"):
        m = copy.deepcopy(m0)
        m._inf_prep = None
        if key == "inf":
            with torch.no_grad():
                m.beta_cim.view(-1)[5] = float("inf")
        assert _supported(m, x) == 1
        m.eval()
        with torch.no_grad():
            got = m.forward_fused(x, one, zero, relu=True)
        buf = m._inf_prep.buf  # (kept until train() drops it)
        flags[key] = int(buf[buf.numel() - 512:buf.numel() - 508].view(torch.int32).item())
        want = _unprepared(m, x, one, zero, relu=True)
        _same(got, want, key)
        outs[key] = got
    assert flags == {"finite": 0, "inf": 1}
    assert not torch.equal(_bits(outs["finite"]), _bits(outs["inf"]))


def test_weight_cache_shift(cuda_device, monkeypatch):
    L = _L()
    m0, x = _layer("w2a2_16", cuda_device)
    assert _supported(m0, x) == 1
    m = copy.deepcopy(m0)
    m._inf_prep = None
    lib = L.load()
    calls, other = [], []
    real, real_lib = lib.cimq_module_prepare_shift, lib.cimq_module_prepare

    def counted(*a):
        calls.append(a[0])
        return real(*a)

    def counted_lib(*a):  # (a shift layer never goes through the library ADC's entry point)
        other.append(a[0])
        return real_lib(*a)
    monkeypatch.setattr(lib, "cimq_module_prepare_shift", counted)
    monkeypatch.setattr(lib, "cimq_module_prepare", counted_lib)
    m.eval()
    with torch.no_grad():
        y1 = m(x)
        assert calls == [1] and m._inf_prep is not None
        y2 = m(x)
        assert calls == [1]  # the second call reuses the cache
        assert torch.equal(_bits(y1), _bits(y2))
        m.beta_cim.add_(0.5 * m.alpha_cim)
        y3 = m(x)
        assert calls == [1, 1]  # an in-place edit of beta bumps its version: prepared again
    fresh = copy.deepcopy(m0)
    fresh._inf_prep = None
    with torch.no_grad():
        fresh.beta_cim.add_(0.5 * fresh.alpha_cim)
    fresh.eval()
    with torch.no_grad():
        yf = fresh(x)
    assert torch.equal(_bits(y3), _bits(yf)) and not torch.equal(_bits(y3), _bits(y1))
    # forward_fused shares the cache; train() drops it; load_state_dict too
    one, zero = torch.ones(m.out_channels, device=cuda_device), torch.zeros(m.out_channels, device=cuda_device)
    n = len(calls)
    with torch.no_grad():
        assert torch.equal(_bits(m.forward_fused(x, one, zero)), _bits(y3))
    assert len(calls) == n
    m.train()
    assert m._inf_prep is None
    m.eval()
    with torch.no_grad():
        m(x)
    assert m._inf_prep is not None and len(calls) == n + 1
    m.load_state_dict(m0.state_dict())
    assert m._inf_prep is None
    with torch.no_grad():
        assert torch.equal(_bits(m(x)), _bits(y1))
    assert other == []


# ---------------------------------------------------------------------------------------------------
# a layer the fused shift path refuses (O = 24)
# ---------------------------------------------------------------------------------------------------
def test_unsupported_layer_keeps_todays_path(cuda_device):
    F, L = _F(), _L()
    m, _, x, *_ = _build(cuda_device, 16, 24, 16, 1, 2, 2, 9800, False)
    x = torch.from_numpy(x).to(cuda_device)
    assert _supported(m, x) == 0 and not m._shift_fused(x)
    it, keep, _ = F._prepare_item(m, tuple(x.shape), inference=True)
    arr = (L.PrepareShiftItem * 1)(it)
    rc = L.load().cimq_module_prepare_shift(1, arr, torch.cuda.current_stream().cuda_stream)
    assert rc == L.CIMQ_EUNSUPPORTED and b"cimq_module_shift_supported" in L.load().cimq_last_error()
    del keep
    # the module evaluates as it does today: the unfused shift entry points, no prepared side kept
    try:
        m.eval()
        with torch.no_grad():
            inf = m(x)
        assert m._inf_prep is None and not m.fused_epilogue_ready(x)
        trn = m(x.clone().requires_grad_(True)).detach()
    finally:
        m.train()
    assert torch.equal(_bits(inf), _bits(trn))


def _shift_net(dev, blocks, widths=(16, 32, 64), seed=3030):
    """the harness ResNet of 6 * blocks + 2 layers, every conv a Conv2dLSQCiM(adc_shift=True) w2a2 on xbar 64 (the
    first conv w8a8), one training-mode step at B = 2 for the first-step initialisation, then random beta and
    BatchNorm statistics, eval().  ``widths``: (16, 32, 64), or a first stage of another width."""
    from cim_quantization_amd._modules.lsq import Conv2dLSQCiM
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    torch.manual_seed(seed)
    model = models.ResNet(blocks)
    if widths[0] != 16:  # a first stage of width 24: 3 -> 24, 24 -> 24, and 24 -> 32 with four zero channels a side
        w = widths[0]
        model.conv1 = torch.nn.Conv2d(3, w, 3, stride=1, padding=1, bias=False)
        model.bn1 = torch.nn.BatchNorm2d(w)
        model.layer1 = torch.nn.Sequential(*[models.BasicBlock(w, w) for _ in range(blocks)])
        first = models.BasicBlock(w, 32, 2)
        first.shortcut = models.PadShortcut((32 - w) // 2)
        model.layer2[0] = first
    ReplaceModuleTool(model, {"Conv2d": [Conv2dLSQCiM]}, replace_first_layer=True, nbits_w=2, nbits_a=2, xbar=64,
                      adcbits=1.5, adc_shift=True).replace()
    model = model.to(dev).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(seed + 1)).to(dev)
    model(x)
    k = 0
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, Conv2dLSQCiM):
                assert mod.adc_shift
                mod.beta_cim.copy_(_beta(mod, seed + 100 + k))
                k += 1
    assert k == 6 * blocks + 1
    randomise_bn(model, seed + 2)
    model.eval()
    return model, x


def test_model_with_an_unsupported_layer_runs_the_loop(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _shift_net(cuda_device, 1, widths=(24, 32, 64))
    assert not model.layer1[0].conv1.fused_epilogue_ready(torch.empty(2, 24, 32, 32, device=cuda_device))
    assert model.layer3[0].conv2.fused_epilogue_ready(torch.empty(2, 64, 8, 8, device=cuda_device))
    with torch.no_grad():
        fused = FusedEval(model, net=True)
        got = fused(x)
        assert fused.net_used is False and fused.net_reason
        assert torch.equal(_bits(got), _bits(FusedEval(model)(x)))


# ---------------------------------------------------------------------------------------------------
# the network
# ---------------------------------------------------------------------------------------------------
_NETS = {}


def _net3(dev):
    if "m" not in _NETS:
        _NETS["m"] = _shift_net(dev, 3)
    return _NETS["m"]


def test_fused_eval_net_shift_resnet20(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _net3(cuda_device)
    lin = model.linear
    with torch.no_grad():
        plane, _ = _loop_last_plane(model, x)
        fused = FusedEval(model, net=True)
        got = fused(x)
        assert fused.net_used is True, fused.net_reason  # (the parent runs the loop here)
        assert fused._net_plan.n_slots == 3
        last = fused._net_plan.last_plane().clone()
        assert torch.equal(_bits(last), _bits(plane))
        assert 0.02 < float((last == 0).float().mean()) < 0.98
        # the logits: inside test_gpu_net's head bars of float64 arithmetic on that plane
        pooled = TF.avg_pool2d(last, last.shape[3]).flatten(1)
        pbar, lbar = _head_bars(last, pooled, lin.weight.detach(), lin.bias.detach())
        mean64 = last.double().cpu().mean(dim=(2, 3))
        want = mean64 @ lin.weight.detach().double().cpu().t() + lin.bias.detach().double().cpu()
        extra = (lin.weight.detach().double().cpu().abs().unsqueeze(0) * pbar.unsqueeze(1)).sum(dim=2)
        err = (got.double().cpu() - want).abs()
        print("net logits: max error %.3e, bar %.3e" % (float(err.max()), float((lbar + extra).max())))
        assert bool((err <= lbar + extra).all())
        assert torch.equal(_bits(fused(x)), _bits(got))  # two runs: equal bits
        # codes on the edges: the same logits, the loop's edges
        fc = FusedEval(model, net=True, codes=True)
        gotc = fc(x)
        assert fc.net_used is True, fc.net_reason
        assert torch.equal(_bits(gotc), _bits(got))
        assert torch.equal(_bits(fc._net_plan.last_plane()), _bits(plane))
        loop = FusedEval(model, codes=True)
        loop(x)
        assert len(fc.code_edges) == 18 and fc.code_edges == loop.code_edges


def test_beta_edit_rebuilds_the_plan(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _net3(cuda_device)
    conv = model.layer2[1].conv2
    b0 = conv.beta_cim.detach().clone()
    try:
        with torch.no_grad():
            fused = FusedEval(model, net=True)
            base = fused(x)
            plan = fused._net_plan
            fused(x)
            assert fused._net_plan is plan
            conv.beta_cim.add_(0.5 * conv.alpha_cim)
            a = fused(x)
            assert fused.net_used and fused._net_plan is not plan
            assert torch.equal(_bits(a), _bits(FusedEval(model, net=True)(x))) and not torch.equal(a, base)
            assert torch.equal(_bits(fused._net_plan.last_plane()), _bits(_loop_last_plane(model, x)[0]))
    finally:
        with torch.no_grad():
            conv.beta_cim.copy_(b0)
    with torch.no_grad():
        assert torch.equal(_bits(fused(x)), _bits(base)) and fused.net_used


def test_validate_net_shift(cuda_device):
    from cim_quantization_amd.harness import train
    model, _ = _net3(cuda_device)
    g = torch.Generator().manual_seed(6)
    batches = [(torch.randn(2, 3, 32, 32, generator=g).to(cuda_device),
                torch.randint(0, 10, (2,), generator=g).to(cuda_device)) for _ in range(2)]

    class HP:
        overfit_test = False

    crit = torch.nn.CrossEntropyLoss()
    from cim_quantization_amd.harness import fuse
    used = []
    orig = fuse.FusedEval.forward

    def spy(self, t):
        y = orig(self, t)
        used.append((self.net, self.net_used))
        return y
    fuse.FusedEval.forward = spy
    try:
        got = train.validate(batches, model, crit, HP, fused=True, net=True)
        assert used == [(True, True)] * 2
        want = train.validate(batches, model, crit, HP, fused=True)
    finally:
        fuse.FusedEval.forward = orig
    # cross-entropy moves by at most twice the largest logit change, and the logits move by the head's error alone
    with torch.no_grad():
        bar = max(_logit_bar(_loop_last_plane(model, bx)[0], model) for bx, _ in batches)
    print("validate: loss %.9g (net) vs %.9g (loop), bound %.3e" % (got[2], want[2], 2 * bar))
    assert abs(got[2] - want[2]) <= 2 * bar


def test_net_launches_shift(cuda_device):
    """one forward's device kernels, all libcimq's: with the prepared weight side and the quantiser in the row
    staging (Route::actq for forward-only shift layers) each of the 18 w2a2 layers is ONE cim_fwd_v3_kernel launch;
    the w8a8 first conv keeps its activation prologue (two launches); the head is one: 21"""
    import importlib.util
    import os

    from conftest import REPO
    from cim_quantization_amd.harness.fuse import FusedEval
    spec = importlib.util.spec_from_file_location("infer_net_bench", os.path.join(REPO, "tools", "infer_net_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    model, x = _net3(cuda_device)
    with torch.no_grad():
        loop, net = FusedEval(model), FusedEval(model, net=True)
        loop(x)
        net(x)
        n_loop = tool.count_launches(lambda: loop(x))
        n_net = tool.count_launches(lambda: net(x))
    assert net.net_used
    assert "error" not in n_loop and "error" not in n_net, (n_loop, n_net)
    print("device kernels per forward: loop %s, net %s" % (n_loop, n_net))
    assert n_net["kernels"] == n_net["libcimq"] == 21
    assert n_net["libcimq"] == n_loop["libcimq"] + 1  # (the loop's layers are prepared and staged too; plus the head)


def test_fused_eval_net_shift_resnet56(cuda_device):
    """depth 9: the plan of 55 layers builds, needs three slots, and its last plane is the loop's"""
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _shift_net(cuda_device, 9, seed=5656)
    with torch.no_grad():
        plane, _ = _loop_last_plane(model, x)
        fused = FusedEval(model, net=True)
        fused(x)
        assert fused.net_used is True, fused.net_reason
        assert fused._net_plan.net.n_layers == 55 and fused._net_plan.n_slots == 3
        assert torch.equal(_bits(fused._net_plan.last_plane()), _bits(plane))
        assert bool(np.isfinite(plane.cpu().numpy()).all())


# ---------------------------------------------------------------------------------------------------
# the launcher
# ---------------------------------------------------------------------------------------------------
def test_launcher_adc_shift(cuda_device, tmp_path, capsys):
    """harness.train --adc-shift at cfg4's settings (w2a2, xbar 64, adc 1.5) on synthetic CIFAR-10 batches: a few
    SGD steps, a checkpoint with the beta_cim keys, an evaluate-only run resumed from it through --fused-net (every
    forward one cimq_net_forward call), and torch's own missing-key error for a checkpoint without the keys"""
    import os

    from cim_quantization_amd.harness import fuse, train
    from test_gpu_harness import PROTO, _data
    proto = PROTO.replace("nbits_w: 3", "nbits_w: 2").replace("nbits_a: 3", "nbits_a: 2").replace("xbar: 128",
                                                                                                 "xbar: 64")
    proto = proto.replace("epochs: 2", "epochs: 1")
    _data(str(tmp_path))
    log = str(tmp_path / "run")
    hp1 = tmp_path / "train.prototxt"
    hp1.write_text(proto.format(log=log, data=str(tmp_path), extra=""))
    best = train.main(["--hp", str(hp1), "--max-steps", "2", "--max-val-steps", "1", "--adc-shift"])
    assert np.isfinite(best) and "epoch 0:" in capsys.readouterr().out
    ck_path = os.path.join(log, "resnet20_Conv2dLSQCiMcheckpoint.pth.tar")
    sd = torch.load(ck_path, map_location="cpu", weights_only=True)["state_dict"]
    assert sum(k.endswith("beta_cim") for k in sd) == 19
    assert sd["layer1.0.conv1.beta_cim"].shape == sd["layer1.0.conv1.alpha_cim"].shape == (1, 3, 2, 2, 1, 16)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    hp2 = tmp_path / "eval.prototxt"
    hp2.write_text(proto.format(log=log, data=str(tmp_path), extra=f'evaluate: true\nresume: "{ck_path}"'))
    used = []
    orig = fuse.FusedEval.forward

    def spy(self, t):
        y = orig(self, t)
        used.append((self.net, self.net_used, self.net_reason))
        return y
    fuse.FusedEval.forward = spy
    try:
        acc_net = train.main(["--hp", str(hp2), "--max-val-steps", "2", "--adc-shift", "--fused-net"])
        assert used == [(True, True, None)] * 2, used
        acc_loop = train.main(["--hp", str(hp2), "--max-val-steps", "2", "--adc-shift", "--fused-eval"])
    finally:
        fuse.FusedEval.forward = orig
    assert np.isfinite(acc_net) and np.isfinite(acc_loop)
    model, _ = train.build_model(train.load_hyperparam(str(hp2)), cuda_device, adc_shift=True)
    assert torch.equal(model.layer3[2].conv2.beta_cim.detach().cpu(), sd["layer3.2.conv2.beta_cim"])
    # a checkpoint without the beta_cim keys
    plain = tmp_path / "plain.pth.tar"
    torch.save({"state_dict": {k: v for k, v in sd.items() if not k.endswith("beta_cim")}}, str(plain))
    hp3 = tmp_path / "plain.prototxt"
    hp3.write_text(proto.format(log=log, data=str(tmp_path), extra=f'evaluate: true\nresume: "{plain}"'))
    with pytest.raises(RuntimeError, match=r"Missing key\(s\) in state_dict.*beta_cim"):
        train.build_model(train.load_hyperparam(str(hp3)), cuda_device, adc_shift=True)
    # ... which loads into a model built without the flag, as before
    train.build_model(train.load_hyperparam(str(hp3)), cuda_device)
