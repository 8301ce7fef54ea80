"""Time of one Conv2dLSQCiM(adcbits=0) layer -- the ideal ADC -- on the library path (functional.cim_ideal_conv:
cimq_ideal_forward / cimq_ideal_backward) and on the torch branch (``fused = False``: torch quantisers, the vendor
conv, autograd), per distinct ResNet-20 conv shape (bench.RESNET20, at w3a3 and w4a4; its first conv at w8a8) and per
VGG-small conv shape (the first conv and tools/wide_layer_bench.py's SHAPES, w3a3 and w4a4), B = 256.

For each shape: forward + backward, and the no-grad forward, each captured as one HIP graph and timed over
``--steps`` replays between two HIP events after a warm-up (w4a4_layer_bench._graph_ms); the two sides alternate over
``--runs`` runs in one session.  Per row the runs, their medians and spreads (max - min) and ``faster_*``: the
library's median is below torch's by more than the larger of the two spreads -- the gate a shape has to pass to stay
in ideal_plan.  ``--wide-backward`` adds a third side to the alternation, the library with ``m.wide_backward = True``
(CIMQ_OPT_WIDE_BWD: the large-layer backward pair where cimq_ideal_wide_plan holds), and ``faster_step_wide_vs_torch``
/ ``faster_step_wide_vs_lib`` by the same rule; ``--nets`` keeps the rows of the named networks.  ``--wide-forward`` is a
mode of its own (measure_wide_forward): the large-layer forward against the generic one, and against the parent
commit's library in a whole forward + backward, on the five large VGG-small shapes.

    python tools/ideal_layer_bench.py --out profiles/ideal/summary.json
    python tools/ideal_layer_bench.py --wide-backward --nets vggsmall --out profiles/ideal_wide/summary.json
    python tools/ideal_layer_bench.py --wide-forward --parent-lib PARENT/libcimq.so --out profiles/ideal_wide_fwd/summary.json
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

from wide_layer_bench import SHAPES as VGG_WIDE  # noqa: E402


def shapes(bits):
    """(net, C, O, H, stride, bits), each once"""
    import bench
    out = []
    for _, c, o, h, s, nb in bench.RESNET20:
        for b in ([8] if nb == 8 else bits):
            row = ("resnet20", c, o, h, s, b)
            if row not in out:
                out.append(row)
    for c, o, h in [(3, 128, 32)] + list(VGG_WIDE):
        for b in ([8] if c == 3 else bits):
            out.append(("vggsmall", c, o, h, 1, b))
    return out


def measure_wide_forward(args):
    """--wide-forward: per large VGG-small shape, in one session and alternating over --runs runs,
    the no-grad forward without the hint (cim_ideal_fwd_kernel) against the same call with it (cim_ideal_fwd_wide_kernel
    where cimq_ideal_wide_fwd_plan holds), and forward + backward with the hint under --parent-lib (the parent commit's
    libcimq.so: the generic forward before the wide backward pair) against this tree's library (the large-layer forward
    before the same pair).  A side wins where its median is below the other's by more than the sum of the two spreads."""
    import torch

    import cim_quantization_amd._lib as L
    import cim_quantization_amd._modules as my_nn
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("ideal_layer_bench measures on a GPU; none found")
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--wide-forward times the step against the parent commit's library: give --parent-lib")
    this = L.load()
    parent = L.load(os.path.abspath(args.parent_lib))
    if hasattr(parent, "cimq_ideal_wide_fwd_abi"):
        raise SystemExit("--parent-lib already has the large-layer forward")
    dev = torch.device("cuda", 0)
    rows = []
    for c, o, h in VGG_WIDE:
        for bits in args.bits:
            torch.manual_seed(11)
            m = my_nn.Conv2dLSQCiM(c, o, 3, 1, 1, bias=False, nbits_w=bits, nbits_a=bits, adcbits=0)
            torch.nn.init.kaiming_normal_(m.weight)
            m = m.to(dev).train()
            x = torch.randn(args.batch, c, h, h, device=dev).relu()
            g = torch.randn(args.batch, o, h, h, device=dev) / math.sqrt(args.batch * o * h * h)
            m(x[:2].contiguous()).backward(g[:2].contiguous())  # the initialising step, on two images (torch path)
            xg = x.clone().requires_grad_(True)

            def step():
                xg.grad = None
                m(xg).backward(g)

            def evalf():
                with torch.no_grad():
                    m(x)

            d = L.make_ideal_desc(args.batch, c, h, h, o, 3, 3, (1, 1), (1, 1), bits, bits,
                                  options=L.CIMQ_OPT_WIDE_BWD)
            plan = L.ideal_wide_fwd_plan(d)
            # (kind, side) -> (library, hint)
            sides = {("eval", "plain"): (this, False), ("eval", "wide"): (this, True),
                     ("step", "parent"): (parent, True), ("step", "wide"): (this, True)}
            us = {k: [] for k in sides}
            try:
                for _ in range(args.runs):
                    for (kind, side), (lib, hint) in sides.items():
                        L._lib, m.wide_backward = lib, hint
                        with torch.enable_grad() if kind == "step" else torch.no_grad():
                            ready = m.ideal_ready(xg if kind == "step" else x)
                        if not ready:
                            raise SystemExit(f"{c}->{o} {h}x{h}: {kind} / {side} is not on the library")
                        us[kind, side].append(1e3 * _graph_ms(step if kind == "step" else evalf, args.steps, args.warmup))
            finally:
                L._lib = this
            row = {"bits": bits, "C": c, "O": o, "H": h, "wide_fwd_plan": list(plan)}
            for kind, base in (("eval", "plain"), ("step", "parent")):
                med = {s: statistics.median(us[kind, s]) for s in (base, "wide")}
                spread = {s: max(us[kind, s]) - min(us[kind, s]) for s in (base, "wide")}
                row.update({f"us_{kind}_{base}": us[kind, base], f"us_{kind}_wide": us[kind, "wide"],
                            f"median_{kind}_{base}": med[base], f"median_{kind}_wide": med["wide"],
                            f"spread_{kind}_{base}": spread[base], f"spread_{kind}_wide": spread["wide"],
                            f"ratio_{kind}": med[base] / med["wide"],
                            f"won_{kind}": med["wide"] < med[base] - (spread[base] + spread["wide"]),
                            f"lost_{kind}": med["wide"] > med[base] + (spread[base] + spread["wide"])})
            rows.append(row)
            print(f"w{bits}a{bits} {c:3d}->{o:3d} {h:2d}x{h:<2d} plan {plan}  no-grad forward plain "
                  f"{row['median_eval_plain']:7.1f} us (+-{row['spread_eval_plain']:.1f}) wide "
                  f"{row['median_eval_wide']:7.1f} us (+-{row['spread_eval_wide']:.1f}) x{row['ratio_eval']:.2f} won "
                  f"{row['won_eval']}  fwd+bwd parent {row['median_step_parent']:7.1f} us "
                  f"(+-{row['spread_step_parent']:.1f}) wide {row['median_step_wide']:7.1f} us "
                  f"(+-{row['spread_step_wide']:.1f}) x{row['ratio_step']:.2f} won {row['won_step']}", flush=True)
            del m, x, xg, g
            torch.cuda.empty_cache()
    out = {"batch": args.batch, "adc": 0, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "launch": "hip_graph", "device": torch.cuda.get_device_name(dev),
           "sides": {"eval_plain": "this library, no hint: cim_ideal_fwd_kernel",
                     "eval_wide": "this library, the hint: cim_ideal_fwd_wide_kernel",
                     "step_parent": "the parent commit's library, the hint: cim_ideal_fwd_kernel + the wide backward pair",
                     "step_wide": "this library, the hint: cim_ideal_fwd_wide_kernel + the wide backward pair"},
           "rule": "won: the wide median is below the other by more than the sum of the two spreads (max - min)",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wide-forward", action="store_true",
                    help="the large-layer forward against the generic one and against --parent-lib instead")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libcimq.so (--wide-forward)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--wide-backward", action="store_true", help="time wide_backward = True as a third side")
    ap.add_argument("--nets", nargs="+", default=["resnet20", "vggsmall"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.wide_forward:
        return measure_wide_forward(args)
    import torch

    import cim_quantization_amd._modules as my_nn
    from w4a4_layer_bench import _graph_ms
    if not torch.cuda.is_available():
        raise SystemExit("ideal_layer_bench measures on a GPU; none found")
    dev = torch.device("cuda", 0)
    rows = []
    sides = [("torch", False, False), ("lib", True, False)] + ([("wide", True, True)] if args.wide_backward else [])
    for net, c, o, h, s, bits in [r for r in shapes(args.bits) if r[0] in args.nets]:
        torch.manual_seed(11)
        m = my_nn.Conv2dLSQCiM(c, o, 3, s, 1, bias=False, nbits_w=bits, nbits_a=bits, adcbits=0)
        torch.nn.init.kaiming_normal_(m.weight)
        m = m.to(dev).train()
        x = torch.randn(args.batch, c, h, h, device=dev).relu()
        ho = (h + 2 - 3) // s + 1
        g = torch.randn(args.batch, o, ho, ho, device=dev) / math.sqrt(args.batch * o * ho * ho)
        m(x[:2].contiguous()).backward(g[:2].contiguous())  # the initialising step, on two images (torch path)
        xg = x.clone().requires_grad_(True)

        def step():
            xg.grad = None
            m(xg).backward(g)

        def evalf():
            with torch.no_grad():
                m(x)

        us = {(k, on): [] for k in ("step", "eval") for on in (False, True)}
        us[("step", "wide")] = []
        ready = ready_wide = None
        for _ in range(args.runs):
            for side, on, wide in sides:
                m.fused, m.wide_backward = on, wide
                if side == "wide":  # (the hint moves the backward alone: the no-grad forward is the lib side's)
                    ready_wide = bool(m.ideal_ready(xg))
                    us[("step", "wide")].append(1e3 * _graph_ms(step, args.steps, args.warmup))
                    continue
                if on:
                    ready = bool(m.ideal_ready(x))
                us[("step", on)].append(1e3 * _graph_ms(step, args.steps, args.warmup))
                us[("eval", on)].append(1e3 * _graph_ms(evalf, args.steps, args.warmup))
        us = {k: v for k, v in us.items() if v}
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = {k: max(v) - min(v) for k, v in us.items()}
        row = {"net": net, "bits": bits, "C": c, "O": o, "H": h, "stride": s, "ideal_ready": ready}
        if args.wide_backward:
            k = ("step", "wide")
            row.update({"ideal_ready_wide": ready_wide, "us_step_wide": us[k], "median_step_wide": med[k],
                        "spread_step_wide": spread[k]})
            for other, name in ((False, "torch"), (True, "lib")):
                row[f"faster_step_wide_vs_{name}"] = med[k] < med[("step", other)] - max(spread[k],
                                                                                         spread[("step", other)])
        for k in ("step", "eval"):
            row.update({f"us_{k}_torch": us[(k, False)], f"us_{k}_lib": us[(k, True)],
                        f"median_{k}_torch": med[(k, False)], f"median_{k}_lib": med[(k, True)],
                        f"spread_{k}_torch": spread[(k, False)], f"spread_{k}_lib": spread[(k, True)],
                        f"faster_{k}": med[(k, True)] < med[(k, False)] - max(spread[(k, False)], spread[(k, True)])})
        rows.append(row)
        print(f"{net} w{bits}a{bits} {c:3d}->{o:3d} {h:2d}x{h:<2d} s{s} ready {ready}  fwd+bwd torch "
              f"{med[('step', False)]:8.1f} us (+-{spread[('step', False)]:.1f}) lib {med[('step', True)]:8.1f} us "
              f"(+-{spread[('step', True)]:.1f}) faster {row['faster_step']}  eval torch {med[('eval', False)]:8.1f} us "
              f"lib {med[('eval', True)]:8.1f} us faster {row['faster_eval']}" +
              (f"  fwd+bwd wide {med[('step', 'wide')]:8.1f} us (+-{spread[('step', 'wide')]:.1f}) ready {ready_wide} "
               f"faster than torch {row['faster_step_wide_vs_torch']} lib {row['faster_step_wide_vs_lib']}"
               if args.wide_backward else ""), flush=True)
        del m, x, xg, g
        torch.cuda.empty_cache()
    out = {"batch": args.batch, "adc": 0, "steps": args.steps, "warmup": args.warmup, "runs": args.runs,
           "launch": "hip_graph", "device": torch.cuda.get_device_name(dev), "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    return out


if __name__ == "__main__":
    main()
