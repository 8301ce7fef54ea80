"""Whole-network evaluation A/B on the MI355X: the harness ResNet-20 with cfg2's settings (w3a3, the w8a8 first
conv, xbar 128, 1.5-bit ADC) on a synthetic batch, eval mode under torch.no_grad(), in ONE process:

  side A  model(x) -- ResNet.forward: every CiM conv a forward-only library call, then BatchNorm, the residual
          add and ReLU as torch kernels;
  side B  FusedEval(model)(x) -- each BatchNorm folded into a per-channel affine and, with the residual add and
          the ReLU, applied in the conv kernel's registers (cimq_module_forward_epilogue).

  side C  (--codes) FusedEval(model, codes=True)(x) -- side B with the activations handed from conv to conv as
          the consumer's low-bit codes, one byte per element (cimq_module_forward_codes).  The rounds then run
          A, B, C, B again: the second B window gives the spread, and the bar is C <= B + spread.

  side D  (--net) FusedEval(model, net=True)(x) -- side B as ONE library call (cimq_net_forward): the plan built
          once, the option-A shortcuts read as views in the conv epilogues, pooling and the classifier in one head
          kernel, no torch kernel and no Python between the launches.  The rounds run A, B, D, B again.
  side E  (--net --codes) FusedEval(model, net=True, codes=True)(x) -- side D with side C's code edges; the rounds
          run A, B, C, D, E, B again.

The two sides alternate (A, B, A again per round); a window is HIP events round ``passes`` forwards, sized to at
least --window seconds; the second A window of a round gives the run-to-run spread.  Reports the time per
forward of both sides, the spread, the device kernel launches of one forward of each (torch.profiler), the
largest logit difference between the two (they are not bit-identical: harness/fuse.py) and
torch.cuda.max_memory_allocated of one forward of each.

    python tools/infer_net_bench.py [--batch 256] [--rounds 7] [--window 0.25]
                                    [--out profiles/inference/infer_net_bench_B256.json]
    python tools/infer_net_bench.py --codes    # -> profiles/inference/infer_net_bench_codes_B256.json
    python tools/infer_net_bench.py --net --codes   # -> profiles/inference/infer_net_bench_net_B256.json

Another network: ``--arch resnet56 --bits 2 --xbar 64 --adc-shift`` is BASELINE cfg4 (w2a2 on xbar 64 with the per-tile
scale + shift ADC; -> profiles/inference/infer_net_bench_shift_B256.json).  ``--baseline-tree DIR``: side B (and its
second window) comes from the package and the libcimq.so of another checkout of this repository, built there
beforehand -- e.g. the parent commit's -- loaded into the same process under another name, on a model of its own
made from the same seed; the other sides are this tree's.  The defaults, and the files they write, are unchanged.

``--arch vggsmall`` is the harness VGG-small (VGG7, five wide 3 x 3 layers, three 2 x 2 max-pools).  ``--pool`` adds
side P, FusedEval(model, pool=True): the max-pools in the store of the convs in front of them; with ``--net`` side D
is FusedEval(model, net=True, pool=True), the whole VGG as one cimq_net_forward_ex call.  The rounds run A, B, P, D, B
again (-> profiles/vgg_pool/infer_net_bench_vggsmall_B256.json).

Needs the GPU: there is no CPU fallback and no number without a run.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from cim_quantization_amd import _lib  # noqa: E402
from cim_quantization_amd._modules.lsq import Conv2dLSQCiM  # noqa: E402
from cim_quantization_amd.harness import models  # noqa: E402
from cim_quantization_amd.harness.fuse import FusedEval  # noqa: E402
from cim_quantization_amd.harness.replace import ReplaceModuleTool  # noqa: E402


def load_baseline(tree):
    """the cim_quantization_amd package of another checkout (with its own libcimq.so), imported as ``cimq_baseline``"""
    import importlib.util
    path = os.path.join(os.path.abspath(tree), "cim_quantization_amd")
    if not os.path.exists(os.path.join(path, "libcimq.so")):
        raise SystemExit(f"infer_net_bench: no libcimq.so in {path} (build that checkout first)")
    spec = importlib.util.spec_from_file_location("cimq_baseline", os.path.join(path, "__init__.py"),
                                                  submodule_search_locations=[path])
    pkg = importlib.util.module_from_spec(spec)
    sys.modules["cimq_baseline"] = pkg
    spec.loader.exec_module(pkg)
    return pkg


def build_model(batch, dev, arch="resnet20", bits=3, xbar=bench.XBAR, adc_shift=False, pkg=None):
    """``pkg``: the package to build the model from (load_baseline); default this tree's"""
    mods, conv_cls, tool_cls = models, Conv2dLSQCiM, ReplaceModuleTool
    if pkg is not None:
        import importlib
        mods = importlib.import_module(pkg.__name__ + ".harness.models")
        conv_cls = importlib.import_module(pkg.__name__ + "._modules.lsq").Conv2dLSQCiM
        tool_cls = importlib.import_module(pkg.__name__ + ".harness.replace").ReplaceModuleTool
    torch.manual_seed(20)
    model = getattr(mods, "cifar10_vggsmall" if arch == "vggsmall" else arch)()
    tool_cls(model, {"Conv2d": [conv_cls]}, True, nbits_w=bits, nbits_a=bits, nbits_alpha=8, wbitslice=1,
             abitslice=1, xbar=xbar, adcbits=bench.ADC, signed_xbar=True, stochastic_quant=False,
             **({"adc_shift": True} if adc_shift else {})).replace()
    model = model.to(dev).train()
    x = torch.randn(batch, 3, 32, 32, generator=torch.Generator().manual_seed(21)).to(dev)
    model(x)  # the first-step initialisation of every layer, and BatchNorm statistics that are not the defaults
    model.eval()
    return model, x


def timed(fn, n):
    """milliseconds per call of fn over n calls, between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def count_launches(fn):
    """device kernels of one call of fn (and how many of them are libcimq's), or None without a profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        names = [n for n in names if not n.lower().startswith(("memcpy", "memset"))]
        return {"kernels": len(names), "libcimq": sum("cimq::" in n for n in names)}
    except Exception as e:  # noqa: BLE001 -- the count is a side figure: the timing does not depend on it
        return {"error": f"{type(e).__name__}: {e}"}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window (at least 0.2)")
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--codes", action="store_true", help="add side C, FusedEval(model, codes=True): A, B, C, B per round")
    ap.add_argument("--net", action="store_true",
                    help="add side D, FusedEval(model, net=True) (with --codes also E, net=True and codes=True)")
    ap.add_argument("--arch", default="resnet20", choices=("resnet20", "resnet32", "resnet44", "resnet56", "vggsmall"))
    ap.add_argument("--pool", action="store_true",
                    help="add side P, FusedEval(model, pool=True) (a VGG's max-pools in the conv kernels); with --net "
                         "side D is net=True, pool=True")
    ap.add_argument("--bits", type=int, default=3, help="weight and activation bits of every conv but the first")
    ap.add_argument("--xbar", type=int, default=bench.XBAR)
    ap.add_argument("--adc-shift", action="store_true", help="Conv2dLSQCiM(adc_shift=True) layers")
    ap.add_argument("--baseline-tree", default=None,
                    help="another checkout of this repository, built: side B runs its package and library")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("infer_net_bench: no ROCm device (there is no CPU fallback; nothing is measured)")
    tag = "_shift" if args.adc_shift else "_net" if args.net else "_codes" if args.codes else ""
    out_path = args.out or os.path.join(REPO, "profiles", "inference", f"infer_net_bench{tag}_B{args.batch}.json")
    if args.arch == "vggsmall" and not args.out:
        out_path = os.path.join(REPO, "profiles", "vgg_pool", f"infer_net_bench_vggsmall_B{args.batch}.json")
    dev = torch.device("cuda:0")
    net_kw = dict(arch=args.arch, bits=args.bits, xbar=args.xbar, adc_shift=args.adc_shift)
    model, x = build_model(args.batch, dev, **net_kw)
    if args.baseline_tree:  # side B from the other checkout: its modules, its FusedEval, its library
        import importlib
        base = load_baseline(args.baseline_tree)
        base_model, _ = build_model(args.batch, dev, pkg=base, **net_kw)
        fused = importlib.import_module("cimq_baseline.harness.fuse").FusedEval(base_model)
    else:
        fused = FusedEval(model)
    sides = {"A": lambda: model(x), "B": lambda: fused(x)}
    order = ("A", "B", "A2")
    if args.codes:
        coded = FusedEval(model, codes=True)
        sides["C"] = lambda: coded(x)
        order = ("A", "B", "C", "B2")
    if args.pool:
        pooled = FusedEval(model, pool=True)
        sides["P"] = lambda: pooled(x)
        order = (order[:-1] if order[-1] == "B2" else ("A", "B")) + ("P", "B2")
    nets = {}
    if args.net:
        nets["D"] = FusedEval(model, net=True, pool=True) if args.pool else FusedEval(model, net=True)
        if args.codes:
            nets["E"] = FusedEval(model, net=True, codes=True)
        for k, f in nets.items():
            sides[k] = (lambda f: lambda: f(x))(f)
        order = order[:-1] + tuple(nets) + ("B2",)
    with torch.no_grad():
        ya, yb = sides["A"](), sides["B"]()
        codes_info = None
        if args.codes:
            yc = sides["C"]()
            codes_info = {"logits_equal_B": bool(torch.equal(yb, yc)), "code_edges": len(coded.code_edges),
                          "edges_codes_only": sum(e[2] == "codes" for e in coded.code_edges)}
            del yc
        pool_info = None
        if args.pool:
            yp = sides["P"]()
            pool_info = {"logits_equal_B": bool(torch.equal(yb, yp)), "pooled": list(pooled.pooled)}
            del yp
        diff = {"max_abs_logit_difference": float((ya - yb).abs().max()), "max_abs_logit": float(ya.abs().max()),
                "top1_agree": float((ya.argmax(1) == yb.argmax(1)).float().mean())}
        net_info = {}
        for k, f in nets.items():
            yd = f(x)
            net_info[k] = {"net_used": bool(f.net_used), "net_reason": f.net_reason,
                           "max_abs_logit_difference_to_B": float((yd - yb).abs().max()),
                           "top1_agree_with_B": float((yd.argmax(1) == yb.argmax(1)).float().mean()),
                           "code_edges": len(f.code_edges)}
            del yd
        del ya, yb
        for fn in sides.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        passes = max(1, int(max(args.window, 0.2) / (timed(sides["A"], 5) * 1e-3) + 1))
        peak, launches = {}, {}
        for key, fn in sides.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            peak[key] = {"max_memory_allocated": torch.cuda.max_memory_allocated(),
                         "above_resident": torch.cuda.max_memory_allocated() - base}
        tot = {k: [] for k in order}
        for _ in range(args.rounds):
            for key in order:
                tot[key].append(timed(sides[key[0]], passes) * 1e3)
        if not args.no_launch_count:  # (after the timing: the profiler stays out of the windows)
            for key, fn in sides.items():
                launches[key] = count_launches(fn)
    med = {k: statistics.median(v) for k, v in tot.items()}
    twin = order[-1]  # the repeated side: the same code, the same call
    spread = max(abs(a - b) for a, b in zip(tot[twin[0]], tot[twin]))
    result = {
        "workload": f"harness {'VGG-small' if args.arch == 'vggsmall' else 'ResNet-' + args.arch[6:]} evaluation forward (model(x) vs FusedEval(model)(x)), eval + no_grad, "
                    f"B = {args.batch}, w{args.bits}a{args.bits} (first conv w8a8), xbar {args.xbar}, adc {bench.ADC}"
                    f"{', scale + shift ADC (adc_shift)' if args.adc_shift else ''}, synthetic input",
        "device": torch.cuda.get_device_name(0), "abi": _lib.ABI_VERSION,
        "passes_per_window": passes, "rounds": args.rounds,
        "forward_us": {k: round(v, 1) for k, v in med.items()},
        "forward_us_windows": {k: [round(t, 1) for t in v] for k, v in tot.items()},
        "spread_us": round(spread, 1),  # the largest |A - A2| (with --codes |B - B2|) of a round
        "B_minus_A_us": round(med["B"] - med["A"], 1),
        "B_not_above_A_by_more_than_spread": bool(med["B"] <= med["A"] + spread),
        "kernel_launches_per_forward": launches,
        "peak_memory_bytes": peak,
        "fused_vs_batchnorm_path": diff,
    }
    if args.baseline_tree:
        result["workload"] += "; side B (and B2) from the baseline checkout's package and libcimq.so, the others from this tree"
        result["B_from_baseline_tree"] = True
    if args.codes:
        result["workload"] += "; side C = FusedEval(model, codes=True)(x)"
        result["abi_minor"] = _lib.ABI_MINOR
        result["C_minus_B_us"] = round(med["C"] - med["B"], 1)
        result["C_not_above_B_by_more_than_spread"] = bool(med["C"] <= med["B"] + spread)
        result["codes"] = codes_info
    if args.pool:
        result["workload"] += "; side P = FusedEval(model, pool=True)(x)"
        result["pool"] = pool_info
        result["P_minus_B_us"] = round(med["P"] - med["B"], 1)
        result["P_below_B_by_more_than_spread"] = bool(med["P"] < med["B"] - spread)
        result["P_above_B_by_more_than_spread"] = bool(med["P"] > med["B"] + spread)
    if args.net:
        result["workload"] += "; side D = FusedEval(model, net=True%s)(x)" % (", pool=True" if args.pool else "") + \
            (", E = net=True, codes=True" if args.codes else "")
        result["net"] = net_info
        for k in nets:
            result[f"{k}_minus_B_us"] = round(med[k] - med["B"], 1)
            result[f"{k}_below_B_by_more_than_spread"] = bool(med[k] < med["B"] - spread)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    keys = ("forward_us", "spread_us", "B_minus_A_us", "kernel_launches_per_forward", "peak_memory_bytes",
            "fused_vs_batchnorm_path") + (("C_minus_B_us", "C_not_above_B_by_more_than_spread", "codes") if args.codes else ())
    if args.pool:
        keys += ("pool", "P_minus_B_us", "P_below_B_by_more_than_spread", "P_above_B_by_more_than_spread")
    if args.net:
        keys += ("net",) + tuple(f"{k}_minus_B_us" for k in nets) + tuple(f"{k}_below_B_by_more_than_spread" for k in nets)
    print(json.dumps({k: result[k] for k in keys}))
    return result


if __name__ == "__main__":
    main()
