"""Per-layer time of the six ResNet-20 conv shapes (bench.RESNET20) at 4 bits in 1-bit slices: B = 256, xbar 128,
adc 1.5, the forward alone and the forward + backward of one Conv2dLSQCiM, each replayed as a HIP graph and timed
with HIP events after a warm-up -- device time, as bench.py --full takes for its extra configurations.

One run measures one library: whichever ``CIMQ_LIB_PATH`` names, else this tree's.  To compare two revisions,
alternate them in child processes of one GPU session, each under its own time limit, and summarise:

    CIMQ_LIB_PATH=<other revision's libcimq.so> python tools/w4a4_layer_bench.py --tag parent --out runs/parent_0.json
    python tools/w4a4_layer_bench.py --tag new --out runs/new_0.json
    ... (parent_1, new_1, ...)
    python tools/w4a4_layer_bench.py --summarise runs --out profiles/w4a4/summary.json

The summary gives, per shape and tag, the median over the runs and their spread (max - min), and the ratio of the
two medians.  The forward-only column has a summary of its own beside it (``eval``, tags ``new`` and ``parent``): both
medians, the larger of the two spreads, and whether the new median is lower than the parent's by more than that --
the gate a forward-only kernel form has to pass to keep a shape.  ``--forward-only`` measures that column alone.
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def shapes():
    """(name, C, O, H, stride) of bench.RESNET20's distinct conv shapes, in the network's order"""
    import bench
    seen, out = set(), []
    for name, c, o, h, s, _ in bench.RESNET20:
        if (c, o, h, s) not in seen:
            seen.add((c, o, h, s))
            out.append((name, c, o, h, s))
    return out


def _event_ms(call, steps):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(steps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def _graph_ms(fn, steps, warmup):
    """device time per call of fn, replayed as one HIP graph: HIP events around ``steps`` replays"""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        fn()
    for _ in range(max(1, warmup)):
        gr.replay()
    ms = _event_ms(gr.replay, steps)
    del gr
    return ms


def measure(args):
    import torch

    import bench
    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("w4a4_layer_bench measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rows = []
    for name, c, o, h, s in shapes():
        torch.manual_seed(11)
        m = my_nn.Conv2dLSQCiM(c, o, 3, s, 1, bias=False, nbits_w=4, nbits_a=4, nbits_alpha=8, wbitslice=1,
                               abitslice=1, xbar=bench.XBAR, adcbits=bench.ADC)
        torch.nn.init.kaiming_normal_(m.weight)
        m = m.to(dev).train()
        x = torch.randn(args.batch, c, h, h, device=dev)
        x = x if c == 3 else x.relu()
        ho = bench.out_hw(h, s)
        g = torch.randn(args.batch, o, ho, ho, device=dev) / math.sqrt(args.batch * o * ho * ho)
        m(x).backward(g)  # the first step: the step sizes and alpha_cim from the data (torch path)
        route = tuple(L.ROUTE_NAMES[v] for v in L.module_route(F.module_descs(m, tuple(x.shape))[0]))

        def fb():
            m(x).backward(g)

        def fwd():
            with torch.no_grad():
                m(x)

        ms_fb = None if args.forward_only else _graph_ms(fb, args.steps, args.warmup)
        ms_f = _graph_ms(fwd, args.steps, args.warmup)
        rows.append({"layer": name, "C": c, "O": o, "H": h, "stride": s, "route": list(route),
                     "ms_fwd_bwd": ms_fb, "ms_fwd": ms_f})
        print(f"{args.tag} {name:16s} {c:3d}->{o:3d} {h:2d}x{h:<2d} s{s} {'/'.join(route):24s} "
              f"fwd+bwd {float('nan') if ms_fb is None else ms_fb:8.4f} ms  fwd {ms_f:8.4f} ms", flush=True)
    res = {"tag": args.tag, "lib": os.path.relpath(L.LIB_PATH), "batch": args.batch, "bits": 4, "xbar": bench.XBAR,
           "adc": bench.ADC, "steps": args.steps, "warmup": args.warmup, "launch": "hip_graph",
           "device": torch.cuda.get_device_name(dev), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


def summarise(args):
    runs = {}
    for p in sorted(glob.glob(os.path.join(args.summarise, "*.json"))):
        with open(p) as f:
            r = json.load(f)
        if "rows" in r and "tag" in r:
            runs.setdefault(r["tag"], []).append(r)
    if not runs:
        raise SystemExit(f"no runs under {args.summarise}")
    first = next(iter(runs.values()))[0]
    out = {k: first[k] for k in ("batch", "bits", "xbar", "adc", "steps", "warmup", "launch", "device")}
    out["runs"] = {t: len(v) for t, v in runs.items()}
    out["layers"] = []
    for i, row in enumerate(first["rows"]):
        e = {k: row[k] for k in ("layer", "C", "O", "H", "stride")}
        for t, v in runs.items():
            e[t] = {"route": v[0]["rows"][i]["route"]}
            for key in ("ms_fwd_bwd", "ms_fwd"):
                xs = [r["rows"][i][key] for r in v if r["rows"][i][key] is not None]
                if xs:
                    e[t][key] = {"median": statistics.median(xs), "spread": max(xs) - min(xs), "runs": xs}
        tags = list(runs)
        if len(tags) == 2:
            a, b = tags
            for key in ("ms_fwd_bwd", "ms_fwd"):
                if key in e[a] and key in e[b]:
                    e[f"{key}_{a}_over_{b}"] = e[a][key]["median"] / e[b][key]["median"]
        if "new" in runs and "parent" in runs:
            # the forward-only column's own summary: the new form keeps a shape whose median is lower than the
            # parent's by more than the larger of the two spreads
            n, q = e["new"]["ms_fwd"], e["parent"]["ms_fwd"]
            bar = max(n["spread"], q["spread"])
            e["eval"] = {"new_median_ms": n["median"], "parent_median_ms": q["median"], "new_spread_ms": n["spread"],
                         "parent_spread_ms": q["spread"], "gain_ms": q["median"] - n["median"], "bar_ms": bar,
                         "speedup": q["median"] / n["median"], "keeps_new_form": q["median"] - n["median"] > bar}
        out["layers"].append(e)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out["layers"], indent=1))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="new", help="the name of the measured library in the output")
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--forward-only", action="store_true", help="time the no-grad forward alone")
    ap.add_argument("--summarise", default=None, metavar="DIR", help="merge the runs under DIR instead of measuring")
    args = ap.parse_args()
    if args.summarise:
        summarise(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
