"""Generate the golden parity vectors under tests/golden/ from the REAL reference.

Run in the build container only (the reference is not present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden.py [case ...]

(with case names: only those are written, and the other fixtures stay byte for byte.)

It imports ``models._modules`` from /root/reference (read-only, unmodified).  The
reference hard-codes CUDA allocations (lsq.py:64,169,336-337) and ``.cuda()``
(lsq.py:169); inside THIS process only, ``torch.cuda.FloatTensor`` and
``Tensor.cuda`` are redirected to the CPU so the library runs as written.  For each
case the script runs the reference, runs the numpy oracle (``oracle/``) on the same
inputs, asserts agreement, and writes inputs + reference outputs as an .npz (data
only: no reference source is stored).
"""
from __future__ import annotations

import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("CIMQ_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

from oracle import cim_oracle as co  # noqa: E402
from oracle import cim_module_oracle as cmo  # noqa: E402


def _install_cpu_shim():
    class _CpuFloatTensor:
        def __new__(cls, *a):
            return torch.FloatTensor(*a)

    torch.cuda.FloatTensor = _CpuFloatTensor
    torch.Tensor.cuda = lambda self, *a, **k: self


def _import_reference():
    _install_cpu_shim()
    sys.path.insert(0, REF)
    import models._modules.lsq as ref  # noqa: E402
    return ref


F32 = np.float32

# (name, dict) -- Function-level cases: x_q / w_q are codes times scales, like the module makes
FUNCTION_CASES = [
    ("fn_adc15_xbar64_artifact", dict(B=2, C=16, O=8, H=8, k=3, s=1, p=1, wb=3, ab=3, wbs=1, abs=1,
                                       xbar=64, adc=1.5, sa=0.08475284, sw=0.29980746, signed=0)),
    ("fn_adc15_xbar128_s2", dict(B=2, C=16, O=16, H=8, k=3, s=2, p=1, wb=3, ab=3, wbs=1, abs=1,
                                  xbar=128, adc=1.5, sa=0.113, sw=0.0731, signed=0)),
    ("fn_adc4", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=3, ab=3, wbs=1, abs=1, xbar=64,
                     adc=4, sa=0.08475284, sw=0.29980746, signed=0)),
    ("fn_adc6_w2a2", dict(B=2, C=8, O=8, H=6, k=3, s=1, p=1, wb=2, ab=2, wbs=1, abs=1, xbar=64,
                          adc=6, sa=0.31, sw=0.17, signed=0)),
    ("fn_adc1", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=3, ab=3, wbs=1, abs=1, xbar=64,
                     adc=1, sa=0.25, sw=0.5, signed=0)),
    ("fn_adc0", dict(B=2, C=8, O=8, H=6, k=3, s=1, p=1, wb=3, ab=3, wbs=1, abs=1, xbar=64,
                     adc=0, sa=0.08475284, sw=0.29980746, signed=0)),
    ("fn_w8a8_signed_first", dict(B=2, C=3, O=16, H=8, k=3, s=1, p=1, wb=8, ab=8, wbs=1, abs=1,
                                  xbar=128, adc=1.5, sa=0.0123, sw=0.00731, signed=1)),
    ("fn_w4a4_bs2", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=4, ab=4, wbs=2, abs=2, xbar=64,
                         adc=1.5, sa=0.0713, sw=0.0913, signed=0)),
    ("fn_linear_1x1", dict(B=8, C=64, O=32, H=1, k=1, s=1, p=0, wb=4, ab=4, wbs=1, abs=1, xbar=32,
                           adc=1.5, sa=0.0571, sw=0.0377, signed=0)),
    ("fn_alpha_equal_nan", dict(B=1, C=8, O=8, H=4, k=3, s=1, p=1, wb=3, ab=3, wbs=1, abs=1,
                                xbar=64, adc=1.5, sa=0.25, sw=0.5, signed=0, alpha_equal=True)),
    # slice widths other than 1: unequal widths on the two sides, bits the width does not divide
    # (int(5 / 2) = 2 slices cover 4 of the 5 bits), 4-bit slices on the signed first-layer form
    ("fn_w6a3_bs21", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=6, ab=3, wbs=2, abs=1, xbar=64,
                          adc=1.5, sa=0.0913, sw=0.0213, signed=0)),
    ("fn_w3a6_bs12", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=3, ab=6, wbs=1, abs=2, xbar=64,
                          adc=1.5, sa=0.0213, sw=0.0913, signed=0)),
    ("fn_w5a5_bs2", dict(B=2, C=16, O=8, H=6, k=3, s=1, p=1, wb=5, ab=5, wbs=2, abs=2, xbar=64,
                         adc=1.5, sa=0.0413, sw=0.0513, signed=0)),
    ("fn_w8a8_bs4", dict(B=2, C=3, O=16, H=8, k=3, s=1, p=1, wb=8, ab=8, wbs=4, abs=4, xbar=128,
                         adc=1.5, sa=0.0123, sw=0.00731, signed=1)),
]

MODULE_CASES = [
    ("mod_resnet_s1", dict(B=2, C=16, O=16, H=8, k=3, s=1, p=1, wb=3, ab=3, xbar=128, adc=1.5,
                           signed_input=False, bias=False)),
    ("mod_first_layer_w8a8", dict(B=2, C=3, O=16, H=8, k=3, s=1, p=1, wb=8, ab=8, xbar=128,
                                  adc=1.5, signed_input=True, bias=False)),
    ("mod_s2_stride2_xbar64", dict(B=2, C=16, O=32, H=8, k=3, s=2, p=1, wb=3, ab=3, xbar=64,
                                   adc=1.5, signed_input=False, bias=False)),
    ("mod_w2a2_adc4", dict(B=2, C=16, O=16, H=6, k=3, s=1, p=1, wb=2, ab=2, xbar=64, adc=4,
                           signed_input=False, bias=False)),
    ("mod_linear_1x1_w4a4", dict(B=8, C=64, O=32, H=1, k=1, s=1, p=0, wb=4, ab=4, xbar=32,
                                 adc=1.5, signed_input=False, bias=False)),
    ("mod_w4a4_bs2", dict(B=2, C=16, O=16, H=8, k=3, s=1, p=1, wb=4, ab=4, wbs=2, abs=2, xbar=128,
                          adc=1.5, signed_input=False, bias=False)),
]


def function_inputs(cfg, seed):
    rng = np.random.default_rng(seed)
    B, C, O, H, k = cfg["B"], cfg["C"], cfg["O"], cfg["H"], cfg["k"]
    qp_a = 2 ** cfg["ab"] - 1
    qn_w, qp_w = co.lsq_weight_params(cfg["wb"])
    sa = np.array([cfg["sa"]], F32)
    sw = np.array([cfg["sw"]], F32)
    r = rng.integers(0, qp_a + 1, size=(B, C, H, H)).astype(F32)
    r[rng.random(r.shape) < 0.3] = 0  # post-ReLU-like zeros
    rw = rng.integers(qn_w, qp_w + 1, size=(O, C, k, k)).astype(F32)
    x_q = (r * sa).astype(F32)
    w_q = (rw * sw).astype(F32)
    nbw, nba = cfg["wb"] // cfg["wbs"], cfg["ab"] // cfg["abs"]
    T = math.ceil(C * k * k / cfg["xbar"])
    if cfg["adc"] in (1, 1.5):
        if cfg.get("alpha_equal"):
            a = np.full((1, T, nbw, nba, 1, O), 0.7, F32)
        else:
            a = (rng.random((1, T, nbw, nba, 1, O)) * 3.0 + 0.05).astype(F32)
            a *= float(sw[0] * sa[0])
        alpha_q = co.alpha_quantize(a.astype(F32), 8)
    else:
        alpha_q = None
    ho = co.out_size(H, k, cfg["p"], cfg["s"])
    g = rng.standard_normal((B, ho * ho, O)).astype(F32)
    bm = co.make_binary_mask(nbw, nba, cfg["wbs"], cfg["abs"])
    return dict(x_q=x_q, w_q=w_q, sa=sa, sw=sw, alpha_q=alpha_q, grad=g, binary_mask=bm,
                signed_act=np.array([float(cfg["signed"])], F32))


def run_reference_function(ref, cfg, inp):
    x = torch.from_numpy(inp["x_q"].copy()).requires_grad_(True)
    w = torch.from_numpy(inp["w_q"].copy()).requires_grad_(True)
    a = None
    if inp["alpha_q"] is not None:
        a = torch.from_numpy(inp["alpha_q"].copy()).requires_grad_(True)
    st, pd = (cfg["s"], cfg["s"]), (cfg["p"], cfg["p"])
    out = ref.get_cim_output_signed.apply(
        x, w, st, pd, (1, 1), cfg["ab"], cfg["abs"], cfg["wb"], cfg["wbs"], cfg["adc"], cfg["xbar"],
        torch.from_numpy(inp["binary_mask"]), a, torch.from_numpy(inp["sw"]),
        torch.from_numpy(inp["sa"]), False, torch.from_numpy(inp["signed_act"]))
    ctx = out.grad_fn
    res = dict(out=out.detach().numpy().copy(), ctx_x_int8=ctx.x_int.numpy().copy(),
               ctx_w_sliced8=ctx.w_unf_sliced.numpy().copy(), ps16=ctx.ps_int.numpy().copy())
    out.backward(torch.from_numpy(inp["grad"]))
    res["grad_x"] = x.grad.numpy().copy()
    res["grad_w"] = w.grad.numpy().copy()
    if a is not None:
        res["grad_alpha"] = a.grad.numpy().copy()
    return res


def _rel_to_terms(mine, ref_val, terms):
    d = np.abs(mine.astype(np.float64) - ref_val.astype(np.float64))
    scale = np.maximum(np.abs(ref_val.astype(np.float64)), terms) + 1e-30
    return float(np.nanmax(d / scale)) if d.size else 0.0


def check_function_case(name, cfg, inp, res):
    st, pd = (cfg["s"], cfg["s"]), (cfg["p"], cfg["p"])
    out, c = co.cim_forward(inp["x_q"], inp["w_q"], st, pd, (1, 1), cfg["ab"], cfg["abs"], cfg["wb"],
                            cfg["wbs"], cfg["adc"], cfg["xbar"], inp["binary_mask"], inp["alpha_q"],
                            inp["sw"], inp["sa"], False, inp["signed_act"])
    assert np.array_equal(c.x_int8, res["ctx_x_int8"]), name
    assert np.array_equal(c.w_sliced8, res["ctx_w_sliced8"]), name
    same = (c.ps16 == res["ps16"]) | (np.isnan(c.ps16) & np.isnan(res["ps16"]))
    rps = np.rint(res["ps16"].astype(np.float64))
    assert np.array_equal(np.rint(c.ps16.astype(np.float64)), rps), name
    frac_equal = float(same.mean())
    if cfg.get("alpha_equal"):
        assert np.isnan(res["out"]).all() and np.isnan(out).all(), name
        print(f"  {name}: alpha all-equal -> NaN output in both")
        return
    gx, gw, ga = co.cim_backward(c, inp["grad"])
    ax, aw, aa = co.cim_backward(c, inp["grad"], absolute=True)
    _, c64 = co.cim_forward(inp["x_q"], inp["w_q"], st, pd, (1, 1), cfg["ab"], cfg["abs"], cfg["wb"],
                            cfg["wbs"], cfg["adc"], cfg["xbar"], inp["binary_mask"], inp["alpha_q"],
                            inp["sw"], inp["sa"], False, inp["signed_act"], return_debug=True)
    out_terms = np.sum(np.abs(c64.adc.astype(np.float64) * inp["binary_mask"]), axis=(1, 2, 3))
    e_out = _rel_to_terms(out, res["out"], out_terms)
    e_gx = _rel_to_terms(gx, res["grad_x"], ax)
    e_gw = _rel_to_terms(gw, res["grad_w"], aw)
    e_ga = 0.0 if ga is None else _rel_to_terms(ga, res["grad_alpha"], aa)
    print(f"  {name}: ps16 bitwise-equal {frac_equal:.4f}  out {e_out:.2e}  gx {e_gx:.2e}  "
          f"gw {e_gw:.2e}  galpha {e_ga:.2e}")
    assert max(e_out, e_gx, e_gw, e_ga) < 1e-5, name
    res["abs_grad_x"], res["abs_grad_w"] = ax, aw
    res["abs_out"] = out_terms.astype(F32)
    if aa is not None:
        res["abs_grad_alpha"] = aa


def module_inputs(cfg, seed):
    rng = np.random.default_rng(seed)
    B, C, O, H, k = cfg["B"], cfg["C"], cfg["O"], cfg["H"], cfg["k"]
    w = (rng.standard_normal((O, C, k, k)) * math.sqrt(2.0 / (C * k * k))).astype(F32)
    xs = []
    for _ in range(2):
        x = rng.standard_normal((B, C, H, H)).astype(F32)
        if not cfg["signed_input"]:
            x = np.maximum(x, 0).astype(F32)
        xs.append(x)
    ho = co.out_size(H, k, cfg["p"], cfg["s"])
    gs = [rng.standard_normal((B, O, ho, ho)).astype(F32) for _ in range(2)]
    return dict(weight=w, x0=xs[0], x1=xs[1], g0=gs[0], g1=gs[1])


def _module_kwargs(cfg):
    return dict(nbits_w=cfg["wb"], nbits_a=cfg["ab"], nbits_alpha=8, wbitslice=cfg.get("wbs", 1),
                abitslice=cfg.get("abs", 1), xbar=cfg["xbar"], adcbits=cfg["adc"], signed_xbar=True,
                stochastic_quant=False)


def run_module(mod, inp):
    """Two training steps: the init step, then a steady-state step (no optimizer)."""
    res = {}
    with torch.no_grad():
        mod.weight.copy_(torch.from_numpy(inp["weight"]))
    mod.train()
    for step in range(2):
        x = torch.from_numpy(inp[f"x{step}"].copy()).requires_grad_(True)
        out = mod(x)
        out.backward(torch.from_numpy(inp[f"g{step}"]))
        p = f"s{step}_"
        res[p + "out"] = out.detach().numpy().copy()
        res[p + "grad_x"] = x.grad.numpy().copy()
        res[p + "grad_weight"] = mod.weight.grad.numpy().copy()
        res[p + "grad_alpha_act"] = mod.alpha_act.grad.numpy().copy()
        res[p + "grad_alpha_weight"] = mod.alpha_weight.grad.numpy().copy()
        res[p + "alpha_act"] = mod.alpha_act.detach().numpy().copy()
        res[p + "alpha_weight"] = mod.alpha_weight.detach().numpy().copy()
        res[p + "signed_act"] = mod.signed_act.numpy().copy()
        if mod.alpha_cim is not None:
            res[p + "grad_alpha_cim"] = mod.alpha_cim.grad.numpy().copy()
            res[p + "alpha_cim"] = mod.alpha_cim.detach().numpy().copy()
        for prm in mod.parameters():
            prm.grad = None
        with torch.no_grad():  # move the scales off their init values before step 2
            mod.alpha_act.mul_(1.07)
            mod.alpha_weight.mul_(0.93)
            if mod.alpha_cim is not None:
                mod.alpha_cim.mul_(torch.linspace(0.8, 1.2, mod.alpha_cim.numel()).view_as(mod.alpha_cim))
    return res


def main(only=()):
    """``only``: the case names to (re)generate; the other fixtures and their manifest entries stay as they are
    (an .npz is a zip archive and carries its time of writing, so a rewrite changes the file, not the data)"""
    ref = _import_reference()
    torch.set_num_threads(4)
    manifest = {}
    if only:
        with open(os.path.join(HERE, "manifest.json")) as f:
            manifest = json.load(f)
    for idx, (name, cfg) in enumerate(FUNCTION_CASES):
        if only and name not in only:
            continue
        inp = function_inputs(cfg, 1000 + idx)
        res = run_reference_function(ref, cfg, inp)
        check_function_case(name, cfg, inp, res)
        arrays = {("in_" + k): v for k, v in inp.items() if v is not None}
        arrays.update({("ref_" + k): v for k, v in res.items()})
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        manifest[name] = dict(kind="function", cfg=cfg, seed=1000 + idx)
    for idx, (name, cfg) in enumerate(MODULE_CASES):
        if only and name not in only:
            continue
        inp = module_inputs(cfg, 2000 + idx)
        st, pd = cfg["s"], cfg["p"]
        rmod = ref.Conv2dLSQCiM(cfg["C"], cfg["O"], (cfg["k"], cfg["k"]), (st, st), (pd, pd), (1, 1),
                                groups=1, bias=cfg["bias"], **_module_kwargs(cfg))
        omod = cmo.OracleConv2dLSQCiM(cfg["C"], cfg["O"], (cfg["k"], cfg["k"]), (st, st), (pd, pd),
                                      (1, 1), groups=1, bias=cfg["bias"], **_module_kwargs(cfg))
        rres = run_module(rmod, inp)
        ores = run_module(omod, inp)
        worst = {}
        for key, rv in rres.items():
            ov = ores[key]
            if rv.dtype.kind == "f":
                d = np.abs(ov.astype(np.float64) - rv.astype(np.float64))
                s = np.abs(rv.astype(np.float64)).max() + 1e-30
                worst[key] = float(d.max() / s)
        # scalar scale grads are sums with heavy cancellation: bound them by the sum of
        # |terms| of their reduction (g_xq*code and g_x*x/s terms), approximated here by
        # 1e-3 of the value's own magnitude; tests/ apply the exact sum-of-|terms| bound.
        bad = {k: v for k, v in worst.items()
               if v > (1e-3 if ("grad_alpha_act" in k or "grad_alpha_weight" in k) else 1e-5)}
        print(f"  {name}: max rel (vs max|ref|) " + ", ".join(f"{k}={v:.1e}" for k, v in worst.items()
                                                             if k.startswith("s1_")))
        assert not bad, (name, bad)
        arrays = {("in_" + k): v for k, v in inp.items()}
        arrays.update({("ref_" + k): v for k, v in rres.items()})
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        manifest[name] = dict(kind="module", cfg=cfg, seed=2000 + idx)
    with open(os.path.join(HERE, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
    print("wrote", len(manifest), "golden cases")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
