"""GPU: the 2 x 2 / stride-2 max pool in the store of cim_fwd_wide_kernel (cimq_module_forward_pool,
Conv2dLSQCiM.forward_fused(pool=2)), the extended network calls (cimq_net_forward_ex: pooled layers, the flatten
head) and FusedEval(pool=True) on VGG-small.  pool_cases.py, B = 2 unless the case says otherwise.

The reference of every pooled plane is F.max_pool2d(conv.forward_fused(x, scale, shift, residual, relu), 2, 2): the
unpooled epilogue instance, which test_gpu_wide.py holds to the oracle, through torch's own pool.  The comparison is
the int32 bit pattern wherever the reference is not NaN and NaN exactly where it is.  Every case asserts its route
(wide) and cimq_module_pool_supported before it launches: on a library without the feature the case stops there.
The head's bar is test_gpu_net._head_bars on the flattened plane: gamma_(C+1) with C = C * H * W features.
"""
import ctypes
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as TF

from conftest import REPO
from pool_cases import CASES, OFF_WIDE, P1, WIDE64
from rect_cases import make_desc, route_names
from test_gpu_epilogue import _fused, _plain, _tables
from test_gpu_net import _head_bars, _mk, _Plan
from test_gpu_rect import _module_data, _modules
from wide_cases import case_id

pytestmark = pytest.mark.gpu
INF = 4


def _F():
    from cim_quantization_amd import functional as F
    return F


def _L():
    import cim_quantization_amd._lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(got, want):
    """int32 bit patterns wherever the reference is not NaN, NaN exactly where it is"""
    nan = torch.isnan(want)
    return got.shape == want.shape and torch.equal(torch.isnan(got), nan) and \
        torch.equal(_bits(got)[~nan], _bits(want)[~nan])


_DATA = {}


def _case(idx, dev):
    from test_gpu_wide import _two_bit_weight_step
    c = CASES[idx]
    if idx not in _DATA:
        _DATA[idx] = _module_data(c, 9900 + idx, step="quantile")
        if c["wb"] == 2:
            _DATA[idx] = _two_bit_weight_step(c, _DATA[idx], 9950 + idx)
    d = _DATA[idx]
    (m,) = _modules(c, d, dev, oracle=False)
    return c, d, m


def _assert_poolable(c, m, x_shape):
    F, L = _F(), _L()
    assert L.load().cimq_pool_abi() == 1
    assert route_names(L, make_desc(L, c, options=INF)) == ("wide", "none", "none")
    di = F.module_descs(m, tuple(x_shape), inference=True)[0]
    assert route_names(L, di)[0] == "wide" and L.module_pool_supported(di) is True


class _RawPool:
    """cimq_module_forward_pool through ctypes on module m's parameters with no prepared weight side; ``out`` has the
    unpooled size and is filled with a sentinel: a pooled call writes its first quarter"""

    def __init__(self, m, x):
        from test_gpu_codes import _Raw
        self.r = _Raw(m, tuple(x.shape))
        self.x = x

    def call(self, scale, shift, res, relu, pool=2):
        L, r = _L(), self.r
        p = lambda u: None if u is None else u.data_ptr()  # noqa: E731
        r.out.fill_(7.0)
        epi = L.make_epilogue(p(scale), p(shift), p(res), relu)
        rc = L.load().cimq_module_forward_pool(r.desc, r.lsq, p(self.x), *[p(u) for u in r.t], ctypes.byref(epi), pool,
                                               p(r.out), p(r.cbuf), p(r.ws), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def pooled(self):
        B, O, Ho, Wo = self.r.out.shape
        n = B * O * (Ho // 2) * (Wo // 2)
        flat = self.r.out.reshape(-1)
        return flat[:n].view(B, O, Ho // 2, Wo // 2).clone(), flat[n:].clone()


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[case_id(c) for c in CASES])
def test_pooled_store(cuda_device, idx):
    L = _L()
    c, d, m = _case(idx, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_poolable(c, m, x.shape)
    assert m.pool_ready(x) is True
    v = _plain(m, x)
    assert float(v.abs().max()) > 0
    scale, shift, res = _tables(v, 880 + idx)
    raw = _RawPool(m, x)
    for kw in (dict(), dict(relu=True), dict(residual=res, relu=True)):
        want = TF.max_pool2d(_fused(m, x, scale, shift, **kw), 2, 2)
        got = _fused(m, x, scale, shift, pool=2, **kw)                    # the prepared weight side
        assert got.shape == want.shape and tuple(got.shape[2:]) == (v.shape[2] // 2, v.shape[3] // 2)
        print("case P%d %s: max |got - want| %.3e" % (idx + 1, sorted(kw), float((got - want).abs().nan_to_num().max())))
        assert _same(got, want), (sorted(kw), float((got - want).abs().nan_to_num().max()))
        assert _same(_fused(m, x, scale, shift, pool=2, **kw), got)          # a second run
        # unprepared, into a sentinel-filled buffer of the unpooled size: the same plane, the tail untouched, twice
        for _ in range(2):
            assert raw.call(scale, shift, kw.get("residual"), kw.get("relu", False)) == 0, L.load().cimq_last_error()
            head, tail = raw.pooled()
            assert _same(head, want) and bool((tail == 7.0).all())
    frac = float((TF.max_pool2d(_fused(m, x, scale, shift, residual=res, relu=True), 2, 2) == 0).float().mean())
    assert 0.005 < frac < 0.95, frac  # (ReLU cuts some whole windows, and not all)
    # pool == 0 is the epilogue call
    assert raw.call(scale, shift, res, True, pool=0) == 0
    assert torch.equal(raw.r.out, _fused(m, x, scale, shift, residual=res, relu=True))


def test_ties_and_nans(cuda_device):
    """scale 0 and shift -0.0: the stored values are the residual's (0 * v - 0.0 + r), which holds +0.0 / -0.0 in all 16
    sign patterns of a window and windows with one NaN at each of the four positions"""
    c, d, m = _case(P1, cuda_device)
    x = torch.from_numpy(d["x"]).to(cuda_device)
    _assert_poolable(c, m, x.shape)
    v = _plain(m, x)
    assert bool(torch.isfinite(v).all())
    B, O, Ho, Wo = v.shape
    scale = torch.zeros(O, device=cuda_device)
    shift = torch.full((O,), -0.0, device=cuda_device)
    g = torch.Generator().manual_seed(4242)
    win = torch.arange(B * O * (Ho // 2) * (Wo // 2)).view(B, O, Ho // 2, Wo // 2)
    kind = win % 24  # 0..15: a sign pattern of zeros; 16..19: one NaN at position kind - 16 among random values; else random
    res = torch.randn(B, O, Ho, Wo, generator=g)
    for pos, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        sub = res[:, :, i::2, j::2]
        neg = ((kind >> pos) & 1).bool()
        sub[kind < 16] = 0.0
        sub[(kind < 16) & neg] = -0.0
        sub[kind == 16 + pos] = float("nan")
    res = res.to(cuda_device)
    for relu in (False, True):
        full = _fused(m, x, scale, shift, residual=res, relu=relu)
        want = TF.max_pool2d(full, 2, 2)
        wb = _bits(want)
        # the reference holds both zeros and NaN windows of each position
        assert int((wb == 0).sum()) > 0 and int(torch.isnan(want).sum()) >= 4
        if not relu:
            assert int((wb == -2 ** 31).sum()) > 0
            assert torch.equal(torch.isnan(want).cpu(), (kind >= 16) & (kind < 20))
        got = _fused(m, x, scale, shift, residual=res, relu=relu, pool=2)
        assert _same(got, want)


def test_refusals_leave_out_untouched(cuda_device):
    L = _L()
    for c in (WIDE64, OFF_WIDE[1]):  # a wide layer 64 columns wide, a v3 layer
        d = _module_data(c, 9990, step="quantile")
        (m,) = _modules(c, d, cuda_device, oracle=False)
        x = torch.from_numpy(d["x"]).to(cuda_device)
        v = _plain(m, x)
        assert m.pool_ready(x) is False
        scale, shift, _ = _tables(v, 991)
        raw = _RawPool(m, x)
        assert raw.call(scale, shift, None, True) == L.CIMQ_EUNSUPPORTED
        assert b"cimq_module_forward_pool" in L.load().cimq_last_error()
        assert bool((raw.r.out == 7.0).all())
        with pytest.raises(RuntimeError, match="pool_ready"):
            _fused(m, x, scale, shift, pool=2)
        assert raw.call(scale, shift, None, True, pool=0) == 0
        assert torch.equal(raw.r.out, _fused(m, x, scale, shift, relu=True))


# ---------------------------------------------------------------------------------------------------
# the network calls
# ---------------------------------------------------------------------------------------------------
class _PlanEx(_Plan):
    """test_gpu_net._Plan through cimq_net_sizes_ex / cimq_net_forward_ex"""

    def run_ex(self, pool, head_flags=0):
        F, L = _F(), _L()
        net = self.pack()
        ext = L.make_net_ext(pool, head_flags)
        fb, cb, wsb = F.net_sizes(net, ext)
        for s in range(len(self.sf)):  # the buffers are exactly what cimq_net_sizes_ex asks for
            assert self.sf[s].numel() * 4 == fb[s] and cb[s] == 0
        ws = torch.empty(max(wsb, 16), device=self.dev, dtype=torch.uint8)
        n = len(self.sf)
        sf = (ctypes.c_void_p * n)(*[u.data_ptr() for u in self.sf])
        sc = (ctypes.c_void_p * n)()
        F.net_forward(net, self.x.data_ptr(), sf, sc, self.logits.data_ptr(), ws.data_ptr(), ext=ext)
        torch.cuda.synchronize()


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_net_narrow_to_wide(cuda_device, with_res):
    """16 -> 128 @16, 128 -> 128 @16 + pool (with_res: adding the first layer's output, the unpooled shape),
    128 -> 32 @8, a flatten head over [2, 32, 8, 8]: every plane the loop's, the logits inside the head's bar"""
    F, L = _F(), _L()
    dev = cuda_device
    x = torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(71)).abs().to(dev)
    m0 = _mk(dev, 16, 128, 1, x, 9911)
    s0, t0, _ = _tables(_plain(m0, x), 72)
    y0 = _fused(m0, x, s0, t0, relu=True)
    m1 = _mk(dev, 128, 128, 1, y0, 9912)
    s1, t1, _ = _tables(_plain(m1, y0), 73)
    d1 = F.module_descs(m1, tuple(y0.shape), inference=True)[0]
    assert route_names(L, F.module_descs(m0, tuple(x.shape), inference=True)[0])[0] != "wide"
    assert route_names(L, d1)[0] == "wide" and L.module_pool_supported(d1)
    res = y0 if with_res else None
    y1 = _fused(m1, y0, s1, t1, residual=res, relu=True, pool=2)
    assert tuple(y1.shape) == (2, 128, 8, 8)
    assert _same(y1, TF.max_pool2d(_fused(m1, y0, s1, t1, residual=res, relu=True), 2, 2))
    m2 = _mk(dev, 128, 32, 1, y1, 9913)
    s2, t2, _ = _tables(_plain(m2, y1), 74)
    y2 = _fused(m2, y1, s2, t2, relu=True)
    g = torch.Generator().manual_seed(75)
    w = (torch.randn(10, 2048, generator=g) / 45).to(dev)
    b = torch.randn(10, generator=g).to(dev)
    runs = []
    try:
        for mod in (m0, m1, m2):
            mod.eval()
        for _ in range(2):
            p = _PlanEx(x)
            a, bb, cc = p.slot(y0.shape), p.slot(y1.shape), p.slot(y2.shape)
            p.layer(m0, x.shape, s0, t0, True, -1, a)
            p.layer(m1, y0.shape, s1, t1, True, a, bb, res_slot=a if with_res else -1)
            p.layer(m2, y1.shape, s2, t2, True, bb, cc)
            p.set_head(cc, w, b, 10)
            p.run_ex([0, L.CIMQ_POOL_MAX2, 0], L.NET_HEAD_FLATTEN)
            runs.append(p)
    finally:
        for mod in (m0, m1, m2):
            mod.train()
    p = runs[0]
    assert torch.equal(_bits(p.sf[0]), _bits(y0)) and torch.equal(_bits(p.sf[1]), _bits(y1))
    assert torch.equal(_bits(p.sf[2]), _bits(y2))
    flat = y2.reshape(2, 2048, 1, 1)
    _, lbar = _head_bars(flat, flat.flatten(1), w, b)
    want = flat.flatten(1).double().cpu() @ w.double().cpu().t() + b.double().cpu()
    err = (p.logits.double().cpu() - want).abs()
    print("flatten head: max logit error %.3e, bar %.3e" % (float(err.max()), float(lbar.max())))
    assert bool((err <= lbar).all())
    assert torch.equal(_bits(runs[1].logits), _bits(p.logits)) and torch.equal(_bits(runs[1].sf[2]), _bits(p.sf[2]))


# ---------------------------------------------------------------------------------------------------
# VGG-small through FusedEval
# ---------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("infer_net_bench", os.path.join(REPO, "tools", "infer_net_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


_VGG = {}


def _vgg7(dev):
    """test_gpu_wide._vgg, built once for the tests below (they change nothing they do not put back)"""
    if "m" not in _VGG:
        from test_gpu_wide import _vgg
        _VGG["m"], _VGG["x"] = _vgg(dev)
    return _VGG["m"], _VGG["x"]


def _vgg_bar(plane, model):
    """the flatten head's logit bar on the last pooled plane, against another summation order of the same head: twice
    the bar of one evaluation"""
    lin = model.classifier
    flat = plane.reshape(plane.shape[0], -1, 1, 1)
    return _head_bars(flat, flat.flatten(1), lin.weight.detach(), lin.bias.detach())[1]


def test_fused_eval_vgg_pool_loop(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _vgg7(cuda_device)
    tool = _tool()
    with torch.no_grad():
        loop, pooled = FusedEval(model), FusedEval(model, pool=True)
        want = loop(x)
        got = pooled(x)
        assert torch.isfinite(want).all() and torch.equal(got, want)
        assert pooled.pooled == ["features.3", "features.10", "features.17"] and loop.pooled == []
        n_loop, n_pool = tool.count_launches(lambda: loop(x)), tool.count_launches(lambda: pooled(x))
        assert "error" not in n_loop and "error" not in n_pool, (n_loop, n_pool)
        print("device kernels per forward: loop %s, pool %s" % (n_loop, n_pool))
        assert n_pool["kernels"] == n_loop["kernels"] - 3 and n_pool["libcimq"] == n_loop["libcimq"] >= 6
        # net=True without pool is what it was: the loop, with a reason
        fn = FusedEval(model, net=True)
        assert torch.equal(fn(x), want) and fn.net_used is False and fn.net_reason


def test_fused_eval_vgg_one_call(cuda_device):
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _vgg7(cuda_device)
    tool = _tool()
    box = {}
    with torch.no_grad():
        loop = FusedEval(model, pool=True)
        conv = model.features[17]
        orig = conv.forward_fused

        def spy(*a, **k):
            box["y"] = orig(*a, **k)
            return box["y"]
        conv.forward_fused = spy
        try:
            want = loop(x)
        finally:
            del conv.forward_fused
        assert tuple(box["y"].shape) == (2, 512, 4, 4) and torch.equal(want, FusedEval(model)(x))
        net = FusedEval(model, net=True, pool=True)
        got = net(x)
        assert net.net_used is True, net.net_reason
        assert net.pooled == ["features.3", "features.10", "features.17"]
        plan = net._net_plan
        assert plan.net.n_layers == 6 and plan.n_slots == 2
        assert torch.equal(_bits(plan.last_plane()), _bits(box["y"]))
        bar = 2 * _vgg_bar(box["y"], model)
        err = (got.double().cpu() - want.double().cpu()).abs()
        print("VGG7 one call: max logit difference to the loop %.3e, bar %.3e" % (float(err.max()), float(bar.max())))
        assert bool((err <= bar).all())
        # the device kernels of one call: the loop's library kernels and the head kernel, nothing of torch's
        n, n_loop = tool.count_launches(lambda: net(x)), tool.count_launches(lambda: loop(x))
        assert "error" not in n and "error" not in n_loop, (n, n_loop)
        print("device kernels per forward: pooled loop %s, one call %s" % (n_loop, n))
        # (the loop's first conv runs its activation prologue; the plan's quantises in its row staging)
        assert n["kernels"] == n["libcimq"] == n_loop["libcimq"], (n, n_loop)
        # the plan is reused, and remade after a BatchNorm statistic changes
        assert torch.equal(_bits(net(x)), _bits(got)) and net._net_plan is plan
        bn = model.features[4]
        keep = bn.running_var.clone()
        try:
            bn.running_var.mul_(1.5)
            got2 = net(x)
            assert net.net_used and net._net_plan is not plan
            assert not torch.equal(got2, got)
            err2 = (got2.double().cpu() - FusedEval(model)(x).double().cpu()).abs()
            assert bool((err2 <= 2 * _vgg_bar(net._net_plan.last_plane(), model)).all())
        finally:
            bn.running_var.copy_(keep)


@pytest.mark.parametrize("O", [128, 16], ids=["vgg_3to128_per_k", "resnet_3to16_one_block"])
def test_first_conv_quantises_in_its_staging(cuda_device, O):
    """a cimq_net_forward_ex plan of a w8a8 first conv alone (3 -> 128 @ 32, VGG's, the per-k form; 3 -> 16 @ 32, the
    ResNets', the one-block w8a8 form): one device kernel, its plane bit for bit the per-layer call's -- which runs the
    activation prologue first -- also for NaN, +-inf, values past the clamp and exact .5 ties"""
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness.fuse import fold_bn
    F, L = _F(), _L()
    model, x0 = _vgg7(cuda_device)
    conv, bn = model.features[0], model.features[1]
    if O == 16:
        torch.manual_seed(61)
        conv = my_nn.Conv2dLSQCiM(3, 16, 3, 1, 1, bias=False, nbits_w=8, nbits_a=8, nbits_alpha=8, wbitslice=1,
                                  abitslice=1, xbar=128, adcbits=1.5, stochastic_quant=False)
        torch.nn.init.kaiming_normal_(conv.weight)
        conv = conv.to(cuda_device).train()
        conv(x0)
        bn = torch.nn.BatchNorm2d(16).to(cuda_device).eval()
        bn.running_mean.normal_(0, 0.1)
    d = F.module_descs(conv, tuple(x0.shape), inference=True)[0]
    assert conv.nbits_a == 8 and route_names(L, d)[0] == "v3"
    assert L.module_forward_form(d) == ((8, 0) if O == 16 else (0, 0))
    sa = float(F.act_code_step(conv.alpha_act, 1.0 / (x0.numel() * 255.0) ** 0.5))
    x = x0.clone()
    flat = x.view(-1)
    flat[0] = flat[-1] = float("nan")
    flat[5], flat[6] = float("inf"), float("-inf")
    flat[100:140] = (torch.arange(40, device=x.device).float() + 0.5) * sa   # ties
    flat[200:210] = 300.0 * sa                                               # past the clamp
    flat[300:310] = -7.25 * sa
    scale, shift = fold_bn(bn)
    scale, shift = scale.to(cuda_device), shift.to(cuda_device)
    for xi in (x0, x):
        want = _fused(conv, xi, scale, shift, relu=True)
        conv.eval()
        p = _PlanEx(xi)
        a = p.slot(want.shape)
        p.layer(conv, xi.shape, scale, shift, True, -1, a)
        p.logits = torch.zeros(1, device=cuda_device)
        p.run_ex([0])
        assert _same(p.sf[a], want), float((p.sf[a] - want).abs().nan_to_num().max())   # no prepared weight side
        wp = F.inference_weights(conv, tuple(xi.shape), None)
        p.items[-1]["lsq"].wprep = wp.buf.data_ptr()
        p.sf[a].fill_(7.0)
        p.run_ex([0])
        assert _same(p.sf[a], want)                                                      # prepared
        net = p.pack()
        ext = L.make_net_ext([0])
        sfp = (ctypes.c_void_p * 1)(p.sf[a].data_ptr())
        ws = torch.empty(max(F.net_sizes(net, ext)[2], 16), device=cuda_device, dtype=torch.uint8)
        n = _tool().count_launches(lambda: F.net_forward(net, xi.data_ptr(), sfp, (ctypes.c_void_p * 1)(), None,
                                                         ws.data_ptr(), ext=ext))
        assert "error" not in n and n["kernels"] == n["libcimq"] == 1, n
        # ... and without an ext the plan is the old call: the prologue and the forward
        n = _tool().count_launches(lambda: F.net_forward(net, xi.data_ptr(), sfp, (ctypes.c_void_p * 1)(), None,
                                                         ws.data_ptr()))
        assert "error" not in n and n["kernels"] == n["libcimq"] == 2, n
        assert _same(p.sf[a], want)
    # (the special values reach the output: the second input's plane is not the first's, and neither is all zero)
    first = _fused(conv, x0, scale, shift, relu=True)
    conv.eval()
    assert float(first.abs().nan_to_num().max()) > 0 and not _same(want, first)


def test_vgg_one_call_is_seven_kernels(cuda_device):
    """FusedEval(vgg, net=True, pool=True) is 7 device kernels, all the library's: six convs -- the w8a8 first conv
    quantises its input in its row staging inside a cimq_net_forward_ex plan -- and the head"""
    from cim_quantization_amd.harness.fuse import FusedEval
    model, x = _vgg7(cuda_device)
    with torch.no_grad():
        net = FusedEval(model, net=True, pool=True)
        net(x)
        assert net.net_used is True, net.net_reason
        n = _tool().count_launches(lambda: net(x))
    assert "error" not in n, n
    print("VGG7 one call: %s" % (n,))
    assert n["kernels"] == n["libcimq"] == 7, n


def test_validate_pool(cuda_device):
    from cim_quantization_amd.harness import train
    model, x = _vgg7(cuda_device)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.randn(2, 3, 32, 32, generator=g).to(cuda_device),
                torch.randint(0, 10, (2,), generator=g).to(cuda_device)) for _ in range(2)]

    class HP:
        overfit_test = False

    crit = torch.nn.CrossEntropyLoss()
    want = train.validate(batches, model, crit, HP, fused=True)
    assert train.validate(batches, model, crit, HP, fused=True, pool=True) == want
    got = train.validate(batches, model, crit, HP, fused=True, net=True, pool=True)
    from cim_quantization_amd.harness.fuse import FusedEval
    bar = 0.0
    with torch.no_grad():
        for xb, _ in batches:
            f = FusedEval(model, net=True, pool=True)
            f(xb)
            assert f.net_used
            bar = max(bar, float(_vgg_bar(f._net_plan.last_plane(), model).max()))
    print("validate: loss %.9g against %.9g, bar %.3e" % (got[2], want[2], 2 * bar))
    assert abs(got[2] - want[2]) <= 2 * bar
    with pytest.raises(ValueError):
        train.validate(batches, model, crit, HP, pool=True)


def test_narrow_vgg_runs_the_loop(cuda_device):
    """a VGG of 16 / 32 channels: no layer is on the wide route, so pool=True pools nothing in-kernel, and
    net=True, pool=True finds no plan -- net_reason names the first pooled layer -- and runs the loop"""
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd.harness import models
    from cim_quantization_amd.harness.fuse import FusedEval
    from cim_quantization_amd.harness.replace import ReplaceModuleTool
    from test_epilogue_host import randomise_bn
    torch.manual_seed(51)
    model = models.VGG(plan=(16, 16, "M", 32, 32, "M"))
    ReplaceModuleTool(model, {"Conv2d": [my_nn.Conv2dLSQCiM]}, True, nbits_w=3, nbits_a=3, nbits_alpha=8, wbitslice=1,
                      abitslice=1, xbar=128, adcbits=1.5, signed_xbar=True, stochastic_quant=False).replace()
    model = model.to(cuda_device).train()
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(52)).to(cuda_device)
    model(x)
    randomise_bn(model, 53)
    model.eval()
    with torch.no_grad():
        want = FusedEval(model)(x)
        fp = FusedEval(model, pool=True)
        assert torch.equal(fp(x), want) and fp.pooled == []
        fn = FusedEval(model, net=True, pool=True)
        assert torch.equal(fn(x), want)
        assert fn.net_used is False and "features.3" in fn.net_reason and "off the wide route" in fn.net_reason
