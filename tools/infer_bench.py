"""Evaluation forward A/B on the MI355X: the 19 CiM convs of ResNet-20 (bench.RESNET20: w3a3, the w8a8 first
conv, xbar 128, 1.5-bit ADC), forward only, in eval mode under torch.no_grad(), in ONE process:

  side A  cimq_module_forward without CIMQ_OPT_INFERENCE -- the training forward that evaluation ran before
          ABI 15 (functional._INFERENCE = False): state words, backward words, backward weight operands, the
          training ctx and workspace, the weight-side prologue on every call;
  side B  the forward-only mode with each layer's weight-side cache warm.

The two sides alternate (A, B, A again per round); a window is HIP events round ``passes`` x 19 calls, sized to
at least --window seconds; the second A window of a round gives the run-to-run spread.  Reports the total and
per-layer microseconds of both sides, the spread, and torch.cuda.max_memory_allocated of one pass of each.
The outputs of the two sides are compared bit for bit before anything is timed.

    python tools/infer_bench.py [--batch 256] [--rounds 7] [--window 0.25] [--out profiles/inference/infer_bench.json]

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
from cim_quantization_amd import _lib, functional as F  # noqa: E402
from cim_quantization_amd._modules.lsq import Conv2dLSQCiM  # noqa: E402


def build_layers(batch, dev):
    layers = []
    for i, (name, c, o, h, s, nb) in enumerate(bench.RESNET20):
        torch.manual_seed(100 + i)
        m = Conv2dLSQCiM(c, o, 3, s, 1, bias=False, nbits_w=nb, nbits_a=nb, nbits_alpha=8, wbitslice=1, abitslice=1,
                         xbar=bench.XBAR, adcbits=bench.ADC, signed_xbar=True, stochastic_quant=False)
        torch.nn.init.kaiming_normal_(m.weight)
        m = m.to(dev).train()
        x = torch.randn(batch, c, h, h, generator=torch.Generator().manual_seed(200 + i))
        x = (x if i == 0 else x.relu()).to(dev)
        m(x)  # the first-step initialisation
        m.eval()
        layers.append((name, m, x))
    return layers


def one_pass(layers):
    for _, m, x in layers:
        m(x)


def timed(fn, n):
    """milliseconds per call of fn over n calls, between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def side(inference):
    F._INFERENCE = bool(inference)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timed window (at least 0.2)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inference", "infer_bench.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench: no ROCm device (there is no CPU fallback; nothing is measured)")
    dev = torch.device("cuda:0")
    layers = build_layers(args.batch, dev)
    routes = {}
    with torch.no_grad():
        # same results first: both sides on the same inputs, bit for bit
        for name, m, x in layers:
            side(False)
            ya = m(x)
            side(True)
            yb = m(x)
            if not torch.equal(ya, yb):
                raise SystemExit(f"infer_bench: {name}: the two sides' outputs differ")
            desc, _ = F._module_descs(tuple(x.shape), m.weight, m.stride, m.padding, m.dilation, m.nbits_a,
                                      m.abitslice, m.nbits_w, m.wbitslice, m.adcbits, m.xbar, m.nbits_alpha, True,
                                      False)
            routes[name] = _lib.ROUTE_NAMES[_lib.module_route(desc)[0]]
        del ya, yb
        # warm up every shape on both sides; size the windows
        for inf in (False, True):
            side(inf)
            for _ in range(3):
                one_pass(layers)
        torch.cuda.synchronize()
        side(False)
        passes = max(1, int(max(args.window, 0.2) / (timed(lambda: one_pass(layers), 5) * 1e-3) + 1))
        # peak memory of one pass of each side
        peak = {}
        for key, inf in (("A", False), ("B", True)):
            side(inf)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            one_pass(layers)
            torch.cuda.synchronize()
            peak[key] = {"max_memory_allocated": torch.cuda.max_memory_allocated(),
                         "above_resident": torch.cuda.max_memory_allocated() - base}
        # totals: A, B, A per round
        tot = {"A": [], "B": [], "A2": []}
        for _ in range(args.rounds):
            for key, inf in (("A", False), ("B", True), ("A2", False)):
                side(inf)
                tot[key].append(timed(lambda: one_pass(layers), passes) * 1e3)
        # per layer, the same alternation
        per = {}
        for name, m, x in layers:
            side(False)
            n = max(10, int(0.02 / (timed(lambda: m(x), 5) * 1e-3)))
            r = {"A": [], "B": [], "A2": []}
            for _ in range(3):
                for key, inf in (("A", False), ("B", True), ("A2", False)):
                    side(inf)
                    r[key].append(timed(lambda: m(x), n) * 1e3)
            per[name] = {k: round(statistics.median(v), 2) for k, v in r.items()}
            per[name]["route"] = routes[name]
    side(True)
    med = {k: statistics.median(v) for k, v in tot.items()}
    spread = max(abs(a - b) for a, b in zip(tot["A"], tot["A2"]))
    result = {
        "workload": f"ResNet-20 CiM convs forward, eval + no_grad, B = {args.batch}, w3a3 (first conv w8a8), "
                    f"xbar {bench.XBAR}, adc {bench.ADC}",
        "device": torch.cuda.get_device_name(0), "abi": _lib.ABI_VERSION,
        "passes_per_window": passes, "rounds": args.rounds,
        "total_us": {k: round(v, 1) for k, v in med.items()},
        "total_us_windows": {k: [round(t, 1) for t in v] for k, v in tot.items()},
        "spread_us": round(spread, 1),  # the largest |A - A2| of a round: the same code, the same call
        "B_minus_A_us": round(med["B"] - med["A"], 1),
        "B_not_above_A_by_more_than_spread": bool(med["B"] <= med["A"] + spread),
        "peak_memory_bytes": peak,
        "per_layer_us": per,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("total_us", "spread_us", "B_minus_A_us", "peak_memory_bytes")}))
    return result


if __name__ == "__main__":
    main()
