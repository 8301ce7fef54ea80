"""Per-layer time of VGG7's five 3 x 3 conv shapes from 128 input channels up (harness.models.VGG: 128 -> 128 @ 32,
128 -> 256 @ 16, 256 -> 256 @ 16, 256 -> 512 @ 8, 512 -> 512 @ 8) at B = 256, xbar 128, adc 1.5, at w3a3 and w4a4 in
1-bit slices: the training forward, the prepared no-grad forward and ``forward_fused`` (folded affine, residual, ReLU)
of one Conv2dLSQCiM, each replayed as a HIP graph and timed with HIP events after a warm-up, in microseconds, plus the
device kernels one call of each launches.

One run measures one library: whichever ``CIMQ_LIB_PATH`` names, else this tree's.  To compare two revisions,
alternate them in child processes of one GPU session, each under its own time limit, and summarise:

    CIMQ_LIB_PATH=<other revision's libcimq.so> python tools/wide_layer_bench.py --tag parent --out runs/parent_0.json
    python tools/wide_layer_bench.py --tag new --out runs/new_0.json
    ... (parent_1, new_1, ...)
    python tools/wide_layer_bench.py --summarise runs --out profiles/wide/summary.json

The summary gives, per shape, precision, column and tag, the median over the runs and their spread (max - min), and
per column whether the new median is lower than the parent's by more than the larger of the two spreads -- the gate a
shape has to pass to stay in wide_plan.

``--pool``: VGG7's three pooled shapes (128 -> 128 @ 32, 256 -> 256 @ 16, 512 -> 512 @ 8) instead:
``forward_fused(pool=2)`` -- the 2 x 2 max pool in the conv kernel's store -- against the pair it replaces,
``forward_fused`` followed by ``F.max_pool2d(., 2, 2)``, both with the folded affine and the ReLU, each a HIP graph,
alternated over ``--runs`` runs (3) in this one session: per layer the medians, the spreads (max - min) and whether the
pooled call is faster, or slower, than the pair by more than the larger spread.

    python tools/wide_layer_bench.py --pool --out profiles/vgg_pool/layers.json
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(128, 128, 32), (128, 256, 16), (256, 256, 16), (256, 512, 8), (512, 512, 8)]
COLUMNS = ("us_train_fwd", "us_eval_fwd", "us_fused")


def measure(args):
    import torch

    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd import functional as F
    from infer_net_bench import count_launches
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("wide_layer_bench measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rows = []
    for bits in args.bits:
        for c, o, h in SHAPES:
            torch.manual_seed(11)
            m = my_nn.Conv2dLSQCiM(c, o, 3, 1, 1, bias=False, nbits_w=bits, nbits_a=bits, nbits_alpha=8, wbitslice=1,
                                   abitslice=1, xbar=128, adcbits=1.5)
            torch.nn.init.kaiming_normal_(m.weight)
            m = m.to(dev).train()
            x = torch.randn(args.batch, c, h, h, device=dev).relu()
            # the first step on two images: the step sizes and alpha_cim from the data (torch path; its partial sums
            # are [B, T, nbw, nba, P, O] fp32, gigabytes at the full batch)
            g2 = torch.randn(2, o, h, h, device=dev) / math.sqrt(2 * o * h * h)
            m(x[:2].contiguous()).backward(g2)
            xg = x.clone().requires_grad_(True)
            route = tuple(L.ROUTE_NAMES[v] for v in L.module_route(F.module_descs(m, tuple(x.shape))[0]))
            scale, shift = torch.randn(o, device=dev), torch.randn(o, device=dev)
            res = torch.randn(args.batch, o, h, h, device=dev)

            def train_fwd():
                m(xg)

            ms_t = _graph_ms(train_fwd, args.steps, args.warmup)
            n_t = count_launches(train_fwd)
            m.eval()
            with torch.no_grad():
                m(x)  # the kept weight side

                def eval_fwd():
                    m(x)

                def fused():
                    m.forward_fused(x, scale, shift, residual=res, relu=True)

                ms_e = _graph_ms(eval_fwd, args.steps, args.warmup)
                ms_f = _graph_ms(fused, args.steps, args.warmup)
                n_e, n_f = count_launches(eval_fwd), count_launches(fused)
            m.train()
            rows.append({"bits": bits, "C": c, "O": o, "H": h, "route": list(route), "us_train_fwd": 1e3 * ms_t,
                         "us_eval_fwd": 1e3 * ms_e, "us_fused": 1e3 * ms_f,
                         "launches": {"train_fwd": n_t, "eval_fwd": n_e, "fused": n_f}})
            print(f"{args.tag} w{bits}a{bits} {c:3d}->{o:3d} {h:2d}x{h:<2d} {'/'.join(route):24s} train fwd "
                  f"{1e3 * ms_t:9.1f} us  eval fwd {1e3 * ms_e:9.1f} us  fused {1e3 * ms_f:9.1f} us  launches "
                  f"{n_t.get('libcimq')}/{n_e.get('libcimq')}/{n_f.get('libcimq')}", flush=True)
            del m, x, xg, res
            torch.cuda.empty_cache()
    out = {"tag": args.tag, "lib": os.path.relpath(L.LIB_PATH), "batch": args.batch, "xbar": 128, "adc": 1.5,
           "steps": args.steps, "warmup": args.warmup, "launch": "hip_graph", "device": torch.cuda.get_device_name(dev),
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


POOL_SHAPES = [(128, 128, 32), (256, 256, 16), (512, 512, 8)]


def measure_pool(args):
    import torch
    import torch.nn.functional as TF

    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from infer_net_bench import count_launches
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("wide_layer_bench measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rows = []
    for bits in args.bits:
        for c, o, h in POOL_SHAPES:
            torch.manual_seed(11)
            m = my_nn.Conv2dLSQCiM(c, o, 3, 1, 1, bias=False, nbits_w=bits, nbits_a=bits, nbits_alpha=8, wbitslice=1,
                                   abitslice=1, xbar=128, adcbits=1.5)
            torch.nn.init.kaiming_normal_(m.weight)
            m = m.to(dev).train()
            x = torch.randn(args.batch, c, h, h, device=dev).relu()
            g2 = torch.randn(2, o, h, h, device=dev) / math.sqrt(2 * o * h * h)
            m(x[:2].contiguous()).backward(g2)  # the first step on two images (see measure)
            scale, shift = torch.randn(o, device=dev), torch.randn(o, device=dev)
            m.eval()
            with torch.no_grad():
                m(x)  # the kept weight side
                if not m.pool_ready(x):
                    raise SystemExit(f"wide_layer_bench --pool: {c} -> {o} @ {h} does not pool in its kernel")

                def pair():
                    TF.max_pool2d(m.forward_fused(x, scale, shift, relu=True), 2, 2)

                def pooled():
                    m.forward_fused(x, scale, shift, relu=True, pool=2)

                equal = bool(torch.equal(TF.max_pool2d(m.forward_fused(x, scale, shift, relu=True), 2, 2),
                                         m.forward_fused(x, scale, shift, relu=True, pool=2)))
                us = {"pair": [], "pooled": []}
                for _ in range(args.runs):
                    us["pair"].append(1e3 * _graph_ms(pair, args.steps, args.warmup))
                    us["pooled"].append(1e3 * _graph_ms(pooled, args.steps, args.warmup))
                n_pair, n_pool = count_launches(pair), count_launches(pooled)
            e = {"bits": bits, "C": c, "O": o, "H": h, "equal": equal,
                 "launches": {"pair": n_pair, "pooled": n_pool}}
            for k, v in us.items():
                e["us_" + k] = {"median": statistics.median(v), "spread": max(v) - min(v), "runs": v}
            bar = max(e["us_pair"]["spread"], e["us_pooled"]["spread"])
            gain = e["us_pair"]["median"] - e["us_pooled"]["median"]
            e["gate"] = {"gain_us": gain, "bar_us": bar, "speedup": e["us_pair"]["median"] / e["us_pooled"]["median"],
                         "faster": gain > bar, "slower": -gain > bar}
            rows.append(e)
            print(f"w{bits}a{bits} {c:3d}->{o:3d} {h:2d}x{h:<2d} conv + max_pool2d {e['us_pair']['median']:9.1f}"
                  f"+-{e['us_pair']['spread']:6.1f} us  pooled store {e['us_pooled']['median']:9.1f}"
                  f"+-{e['us_pooled']['spread']:6.1f} us  gain {gain:8.1f} us  faster {e['gate']['faster']}  "
                  f"slower {e['gate']['slower']}  equal {equal}", flush=True)
            del m, x
            torch.cuda.empty_cache()
    out = {"lib": os.path.relpath(L.LIB_PATH), "batch": args.batch, "xbar": 128, "adc": 1.5, "steps": args.steps,
           "warmup": args.warmup, "runs": args.runs, "launch": "hip_graph",
           "device": torch.cuda.get_device_name(dev), "layers": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


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
    out = {k: first[k] for k in ("batch", "xbar", "adc", "steps", "warmup", "launch", "device")}
    out["runs"] = {t: len(v) for t, v in runs.items()}
    out["layers"] = []
    for i, row in enumerate(first["rows"]):
        e = {k: row[k] for k in ("bits", "C", "O", "H")}
        for t, v in runs.items():
            e[t] = {"route": v[0]["rows"][i]["route"], "launches": v[0]["rows"][i]["launches"]}
            for key in COLUMNS:
                xs = [r["rows"][i][key] for r in v]
                e[t][key] = {"median": statistics.median(xs), "spread": max(xs) - min(xs), "runs": xs}
        if "new" in runs and "parent" in runs:
            e["gate"] = {}
            for key in COLUMNS:
                n, q = e["new"][key], e["parent"][key]
                bar = max(n["spread"], q["spread"])
                e["gate"][key] = {"gain_us": q["median"] - n["median"], "bar_us": bar,
                                  "speedup": q["median"] / n["median"], "faster": q["median"] - n["median"] > bar}
        out["layers"].append(e)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for e in out["layers"]:
        line = f"w{e['bits']}a{e['bits']} {e['C']:3d}->{e['O']:3d} @{e['H']:2d}"
        for t in runs:
            line += f" | {t} " + " ".join(f"{e[t][k]['median']:9.1f}+-{e[t][k]['spread']:6.1f}" for k in COLUMNS)
        if "gate" in e:
            line += " | faster " + " ".join(str(e["gate"][k]["faster"]) for k in COLUMNS)
        print(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tag", default="new", help="the name of the measured library in the output")
    ap.add_argument("--out", default=None, help="JSON file to write")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--summarise", default=None, metavar="DIR", help="merge the runs under DIR instead of measuring")
    ap.add_argument("--pool", action="store_true",
                    help="time forward_fused(pool=2) against forward_fused + F.max_pool2d on VGG7's pooled shapes")
    ap.add_argument("--runs", type=int, default=3, help="--pool: alternated runs of the two sides")
    args = ap.parse_args()
    if args.pool:
        measure_pool(args)
    elif args.summarise:
        summarise(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
