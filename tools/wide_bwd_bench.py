"""Forward + backward time of VGG7's five wide conv shapes (tools/wide_layer_bench.py's SHAPES) at B = 256, xbar 128,
adc 1.5, at w3a3 and w4a4 in 1-bit slices, with Conv2dLSQCiM.wide_backward off -- the general backward behind the wide
forward, what every call does without the option -- and on: the state-writing forward, cim_bwd_gx_wide_kernel and
cim_bwd_gw_wide_kernel.  One library, one session; the two sides alternate over ``--runs`` runs.  Each run captures
one forward + backward of one module as a HIP graph and times ``--steps`` replays between two HIP events after a
warm-up (w4a4_layer_bench._graph_ms).  Per shape: the medians, the spreads (max - min), the peak device memory of an
eager call on either side, and ``faster``: the option's median is below the other by more than the larger of the two
spreads -- the gate a shape has to pass to stay in wide_bwd_plan.

``--step``: one VGG-small training step through the harness instead -- harness.train's model (build_model on a w3a3
prototxt), optimiser and step body (forward, loss, zero_grad, backward, SGD step) on a synthetic CIFAR batch of
``--batch`` images, eager, HIP events around ``--steps`` steps, the two sides alternated likewise by setting
``wide_backward`` on every CiM conv (what ``--wide-backward`` does).

    python tools/wide_bwd_bench.py --out profiles/wide_bwd/summary.json
    python tools/wide_bwd_bench.py --step --out profiles/wide_bwd/step.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wide_layer_bench import SHAPES  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", action="store_true", help="a VGG-small training step through the harness instead")
    args = ap.parse_args(argv)
    if args.step:
        return measure_step(args)
    import torch

    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from cim_quantization_amd import functional as F
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("wide_bwd_bench measures on a GPU; none found")
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
                torch.cuda.reset_peak_memory_stats(dev)
                step()
                torch.cuda.synchronize()
                peak_b = torch.cuda.max_memory_allocated(dev)
                route = tuple(L.ROUTE_NAMES[v] for v in L.module_route(F.module_descs(m, tuple(x.shape))[0]))
                return 1e3 * _graph_ms(step, args.steps, args.warmup), peak_b, route

            us = {False: [], True: []}
            peak, route = {}, {}
            for _ in range(args.runs):
                for on in (False, True):
                    t, p, r = timed(on)
                    us[on].append(t)
                    peak[on], route[on] = p, r
            med = {k: statistics.median(v) for k, v in us.items()}
            spread = {k: max(v) - min(v) for k, v in us.items()}
            row = {"bits": bits, "C": c, "O": o, "H": h, "route_off": list(route[False]), "route_on": list(route[True]),
                   "us_off": us[False], "us_on": us[True], "median_off": med[False], "median_on": med[True],
                   "spread_off": spread[False], "spread_on": spread[True], "peak_bytes_off": peak[False],
                   "peak_bytes_on": peak[True],
                   "faster": med[True] < med[False] - max(spread.values())}
            rows.append(row)
            print(f"w{bits}a{bits} {c:3d}->{o:3d} {h:2d}x{h:<2d} off {med[False]:9.1f} us (+-{spread[False]:.1f}) "
                  f"{'/'.join(route[False])}  on {med[True]:9.1f} us (+-{spread[True]:.1f}) {'/'.join(route[True])}  "
                  f"peak {peak[False] / 2**20:.0f} / {peak[True] / 2**20:.0f} MiB  faster {row['faster']}", flush=True)
            del m, x, xg, g
            torch.cuda.empty_cache()
    out = {"batch": args.batch, "xbar": 128, "adc": 1.5, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "launch": "hip_graph", "device": torch.cuda.get_device_name(dev), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


PROTO = """
arch: "cifar10_vggsmall"
model_source: Local
log_name: "unused"
data: "unused"
lr: 0.01
epochs: 1
batch_size: {batch}
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
"""


def measure_step(args):
    import tempfile

    import torch
    from torch import nn

    from cim_quantization_amd.harness import train
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
    x = torch.randn(args.batch, 3, 32, 32, device=dev)
    y = torch.randint(0, 10, (args.batch,), device=dev)
    convs = [m for m in model.modules() if hasattr(m, "wide_backward")]

    def step(xb, yb):  # harness.train.train_epoch's step body
        loss = criterion(model(xb), yb)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

    step(x[:2].contiguous(), y[:2].contiguous())  # the initialising step, on two images (torch path)

    def timed(on):
        for m in convs:
            m.wide_backward = on
        for _ in range(args.warmup):
            step(x, y)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            step(x, y)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps, torch.cuda.max_memory_allocated(dev)

    ms, peak = {False: [], True: []}, {}
    for _ in range(args.runs):
        for on in (False, True):
            t, peak[on] = timed(on)
            ms[on].append(t)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: max(v) - min(v) for k, v in ms.items()}
    out = {"arch": arch, "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "launch": "eager, HIP events around the steps", "device": torch.cuda.get_device_name(dev),
           "ms_off": ms[False], "ms_on": ms[True], "median_off": med[False], "median_on": med[True],
           "spread_off": spread[False], "spread_on": spread[True], "peak_bytes_off": peak[False],
           "peak_bytes_on": peak[True], "faster": med[True] < med[False] - max(spread.values())}
    print(f"{arch} B = {args.batch} training step: off {med[False]:.2f} ms (+-{spread[False]:.2f})  on {med[True]:.2f} ms "
          f"(+-{spread[True]:.2f})  peak {peak[False] / 2**20:.0f} / {peak[True] / 2**20:.0f} MiB  faster {out['faster']}",
          flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
