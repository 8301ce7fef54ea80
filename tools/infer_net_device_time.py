"""Where a fused evaluation forward spends its time, on the MI355X: for sides B = FusedEval(model),
C = FusedEval(model, codes=True), D = FusedEval(model, net=True) and E = FusedEval(model, net=True, codes=True) of
tools/infer_net_bench.py (same network, same batch, eval + no_grad),

  * the host time to issue one forward with the device left behind (50 forwards, no synchronisation inside) and
    the wall time per forward of the same loop once the device has drained;
  * the device kernel time of one forward (torch.profiler over 5 forwards, summed per kernel name).

infer_net_bench.py's windows say how long a forward takes end to end; this says whether that is the host or the
device.  It is a profiler run, not a kernel trace with counters.

    python tools/infer_net_device_time.py [--batch 256] [--out profiles/inference/infer_net_device_time_B256.json]

``--arch resnet56 --bits 2 --xbar 64 --adc-shift`` and ``--baseline-tree DIR`` as tools/infer_net_bench.py takes them
(-> profiles/inference/infer_net_device_time_shift_B256.json; side B then comes from the other checkout).

Needs the GPU: there is no CPU fallback and no number without a run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import infer_net_bench as nb  # noqa: E402
from cim_quantization_amd import _lib  # noqa: E402
from cim_quantization_amd.harness.fuse import FusedEval  # noqa: E402


def measure(fn, x, issue=50, profiled=5):
    from torch.profiler import ProfilerActivity, profile
    for _ in range(5):
        fn(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(issue):
        fn(x)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(profiled):
            fn(x)
        torch.cuda.synchronize()
    per = {}
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA or e.name.lower().startswith(("memcpy", "memset")):
            continue
        name = e.name.split("(")[0][:72]
        per[name] = per.get(name, 0.0) + e.device_time / profiled
    top = sorted(per.items(), key=lambda kv: -kv[1])
    return {"host_issue_us": round((t1 - t0) / issue * 1e6, 1), "wall_us": round((t2 - t0) / issue * 1e6, 1),
            "device_kernel_us": round(sum(per.values()), 1),
            "device_kernel_us_by_name": {k: round(v, 1) for k, v in top[:10]}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--arch", default="resnet20", choices=("resnet20", "resnet32", "resnet44", "resnet56"))
    ap.add_argument("--bits", type=int, default=3)
    ap.add_argument("--xbar", type=int, default=nb.bench.XBAR)
    ap.add_argument("--adc-shift", action="store_true")
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("infer_net_device_time: no ROCm device (there is no CPU fallback; nothing is measured)")
    out_path = args.out or os.path.join(REPO, "profiles", "inference",
                                        f"infer_net_device_time{'_shift' if args.adc_shift else ''}_B{args.batch}.json")
    net_kw = dict(arch=args.arch, bits=args.bits, xbar=args.xbar, adc_shift=args.adc_shift)
    model, x = nb.build_model(args.batch, torch.device("cuda:0"), **net_kw)
    loop = FusedEval(model)
    if args.baseline_tree:  # side B from the other checkout: its modules, its FusedEval, its library
        import importlib
        base = nb.load_baseline(args.baseline_tree)
        base_model, _ = nb.build_model(args.batch, torch.device("cuda:0"), pkg=base, **net_kw)
        loop = importlib.import_module("cimq_baseline.harness.fuse").FusedEval(base_model)
    with torch.no_grad():
        sides = {"B": measure(loop, x), "C": measure(FusedEval(model, codes=True), x),
                 "D": measure(FusedEval(model, net=True), x), "E": measure(FusedEval(model, net=True, codes=True), x)}
    default = (args.arch, args.bits, args.xbar, args.adc_shift, args.baseline_tree) == ("resnet20", 3, nb.bench.XBAR, False, None)
    cfg = "" if default else (f" (w{args.bits}a{args.bits}, xbar {args.xbar}{', adc_shift' if args.adc_shift else ''}"
                              f"{'; side B from the baseline checkout' if args.baseline_tree else ''})")
    result = {"workload": f"harness ResNet-{args.arch[6:]}{cfg} fused evaluation forward, B = {args.batch}: B = FusedEval(model), "
                          "C = FusedEval(model, codes=True), D = FusedEval(model, net=True), E = net=True and codes=True; "
                          "host issue and wall over 50 forwards, device kernel time "
                          "from torch.profiler over 5 forwards",
              "device": torch.cuda.get_device_name(0), "abi": [_lib.ABI_VERSION, _lib.ABI_MINOR], "sides": sides}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(sides))
    return result


if __name__ == "__main__":
    main()
