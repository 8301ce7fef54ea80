"""Forward + backward time of the w8a8 first conv beyond 16 output channels -- 3 -> 32, 3 -> 64 and 3 -> 128 at 32 x 32,
B = 256, xbar 128, adc 1.5, 1-bit slices, a signed input -- with Conv2dLSQCiM.wide_backward off (the general recompute
backward, what every call does without the option) and on (cim_bwd_c1w_kernel).  One library, one session; the two
sides alternate over ``--runs`` runs.  Each run captures one forward + backward of the module as a HIP graph and times
``--steps`` replays between two HIP events after a warm-up (w4a4_layer_bench._graph_ms).  Per shape: the medians, the
spreads (max - min) and ``faster``: the option's median is below the other by more than the larger of the two spreads
-- the gate a shape has to pass to stay in c1w_plan.

``--step``: one VGG-small ``--wide-backward`` training step (wide_bwd_bench.measure_step's model, optimiser and step
body, every CiM conv with the option) under this tree's library and under ``--parent-lib`` (the parent commit's
libcimq.so, handed to a fresh child process as CIMQ_LIB_PATH), alternated ``--runs`` times.  A library without the
route trains the first conv on the general backward, so the difference is the route's.

    python tools/c1w_bench.py --out profiles/c1w/summary.json
    python tools/c1w_bench.py --step --parent-lib PARENT/libcimq.so --out profiles/c1w/step.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(3, 32, 32), (3, 64, 32), (3, 128, 32)]  # (C, O, H = W)


def _dump(out, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
    return out


def measure_layers(args):
    import torch

    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd import functional as F
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("c1w_bench measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rows = []
    for c, o, h in SHAPES:
        torch.manual_seed(11)
        m = my_nn.Conv2dLSQCiM(c, o, 3, 1, 1, bias=False, nbits_w=8, nbits_a=8, nbits_alpha=8, wbitslice=1, abitslice=1,
                               xbar=128, adcbits=1.5)
        torch.nn.init.kaiming_normal_(m.weight)
        m = m.to(dev).train()
        x = torch.randn(args.batch, c, h, h, device=dev)  # the normalised image: signed
        g = torch.randn(args.batch, o, h, h, device=dev) / math.sqrt(args.batch * o * h * h)
        m(x[:2].contiguous()).backward(g[:2].contiguous())  # the initialising step, on two images (torch path)
        xg = x.clone().requires_grad_(True)

        def step():
            xg.grad = None
            m(xg).backward(g)

        def timed(on):
            m.wide_backward = on
            step()
            torch.cuda.synchronize()
            route = tuple(L.ROUTE_NAMES[v] for v in L.module_route(F.module_descs(m, tuple(x.shape))[0]))
            return 1e3 * _graph_ms(step, args.steps, args.warmup), route

        us, route = {False: [], True: []}, {}
        for _ in range(args.runs):
            for on in (False, True):
                t, route[on] = timed(on)
                us[on].append(t)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        plan = L.module_c1w_plan(F.module_descs(m, tuple(x.shape))[0])
        rows.append({"C": c, "O": o, "H": h, "route_off": list(route[False]), "route_on": list(route[True]),
                     "plan_ok_groups_blocks_steps": list(plan), "us_off": us[False], "us_on": us[True],
                     "median_off": med[False], "median_on": med[True], "spread_off": spread[False],
                     "spread_on": spread[True], "faster": med[True] < med[False] - max(spread.values())})
        print(f"w8a8 {c}->{o:3d} {h}x{h} off {med[False]:9.1f} us (+-{spread[False]:.1f}) {'/'.join(route[False])}  on "
              f"{med[True]:9.1f} us (+-{spread[True]:.1f}) {'/'.join(route[True])}  plan {plan}  faster "
              f"{rows[-1]['faster']}", flush=True)
        del m, x, xg, g
        torch.cuda.empty_cache()
    return _dump({"batch": args.batch, "xbar": 128, "adc": 1.5, "steps": args.steps, "warmup": args.warmup,
                  "runs": args.runs, "launch": "hip_graph", "device": torch.cuda.get_device_name(dev), "rows": rows},
                 args.out)


def step_child(args):
    """one process, one library (CIMQ_LIB_PATH or the tree's): ms per VGG-small --wide-backward step, as JSON"""
    import tempfile

    import torch
    from torch import nn

    import cim_quantization_amd._lib as L
    from cim_quantization_amd import functional as F
    from cim_quantization_amd.harness import train
    from wide_bwd_bench import PROTO
    dev = torch.device("cuda", 0)
    with tempfile.NamedTemporaryFile("w", suffix=".prototxt") as f:
        f.write(PROTO.format(batch=args.batch))
        f.flush()
        hp = train.load_hyperparam(f.name)
    train.set_seed(hp)
    model, arch = train.build_model(hp, dev)
    criterion = nn.CrossEntropyLoss().to(dev)
    optimizer = train.get_optimizer(model, hp)
    model.train()
    convs = [m for m in model.modules() if hasattr(m, "wide_backward")]
    for m in convs:
        m.wide_backward = True
    x = torch.randn(args.batch, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (args.batch,), device=dev)

    def step(xb, yb):  # harness.train.train_epoch's step body
        loss = criterion(model(xb), yb)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

    step(x[:2].contiguous(), y[:2].contiguous())  # the initialising step, on two images (torch path)
    for _ in range(args.warmup):
        step(x, y)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.steps):
        step(x, y)
    e1.record()
    torch.cuda.synchronize()
    first = next(m for m in convs if m.in_channels == 3)
    route = [L.ROUTE_NAMES.get(v, str(v)) for v in L.module_route(F.module_descs(first, tuple(x.shape))[0])]
    print(json.dumps({"ms": e0.elapsed_time(e1) / args.steps, "arch": arch, "first_conv_route": route,
                      "device": torch.cuda.get_device_name(dev)}), flush=True)


def measure_step(args):
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--step compares against the parent commit's library: give --parent-lib")
    cmd = [sys.executable, os.path.abspath(__file__), "--step-child", "--batch", str(args.batch), "--steps",
           str(args.steps), "--warmup", str(args.warmup)]
    res = {"parent": [], "this": []}
    for _ in range(args.runs):
        for side in ("parent", "this"):
            env = dict(os.environ)
            env.pop("CIMQ_LIB_PATH", None)
            if side == "parent":
                env["CIMQ_LIB_PATH"] = os.path.abspath(args.parent_lib)
            p = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300)
            res[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
    ms = {k: [r["ms"] for r in v] for k, v in res.items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    out = {"arch": res["this"][0]["arch"], "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
           "runs": args.runs, "launch": "eager, HIP events around the steps, a fresh process per library and run",
           "device": res["this"][0]["device"], "first_conv_route_parent": res["parent"][0]["first_conv_route"],
           "first_conv_route_this": res["this"][0]["first_conv_route"], "ms_parent": ms["parent"], "ms_this": ms["this"],
           "median_parent": med["parent"], "median_this": med["this"], "spread_parent": spread["parent"],
           "spread_this": spread["this"], "faster": med["this"] < med["parent"] - max(spread.values())}
    print(f"{out['arch']} B = {args.batch} --wide-backward step: parent {med['parent']:.2f} ms (+-{spread['parent']:.2f}) "
          f"{'/'.join(out['first_conv_route_parent'])}  this {med['this']:.2f} ms (+-{spread['this']:.2f}) "
          f"{'/'.join(out['first_conv_route_this'])}  faster {out['faster']}", flush=True)
    return _dump(out, args.out)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="the VGG-small training step against --parent-lib instead")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libcimq.so")
    ap.add_argument("--step-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.step_child:
        return step_child(args)
    return measure_step(args) if args.step else measure_layers(args)


if __name__ == "__main__":
    main()
