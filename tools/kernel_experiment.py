#!/usr/bin/env python
"""Time libcimq kernels of one ResNet-20 layer shape for several experiment builds.

    python tools/kernel_experiment.py --build            # (CPU) compile the variant libraries
    python tools/kernel_experiment.py --layer layer1.0.conv1   # (GPU) time them

Variant libraries live in exp/ (git-ignored); they skip parts of a kernel to attribute its
time and give wrong results by design -- never used by the product path or the tests.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# name -> preprocessor defines.  The attribution knobs of every round so far (defines that compiled a kernel
# without one of its parts -- the forward without its ADC or its staging, grad_x without its MFMAs, gw5 without
# its global reads, ... -- for timing, wrong results by design) and the tried-and-dropped variants (gx5's DPP
# shifts, the fused kernel's deeper prefetch, ...) are no longer in the shipped kernel sources; an attribution
# run adds its #ifdef to a scratch copy of the kernel and its define here.  Their measurements are in
# DESIGN.md section 4.  What stays are value knobs the sources still read.
VARIANTS = {
    "base": [],
    "cur": [],  # the working tree (a copy of base built later)
    "fold_xb4": ["CIMQ_FOLD_XB=4"],  # round 6: the grad_x folds' x loads four elements per thread at a time
}
if os.environ.get("CIMQ_EXP_VARIANTS"):
    VARIANTS = {k: v for k, v in VARIANTS.items() if k in os.environ["CIMQ_EXP_VARIANTS"].split(",")}


def lib_path(name):
    return os.path.join(REPO, os.environ.get("CIMQ_EXP_DIR", "exp"), f"libcimq_{name}.so")


def do_build():
    from cim_quantization_amd import build as B
    os.makedirs(os.path.dirname(lib_path("base")), exist_ok=True)
    with cf.ThreadPoolExecutor(len(VARIANTS)) as ex:
        futs = {ex.submit(B.build, True, False, lib_path(n), list(d) + ["CIMQ_TUNING"]): n
                for n, d in VARIANTS.items()}
        for f in cf.as_completed(futs):
            f.result()
            print("built", futs[f], flush=True)


def do_time(layer, iters):
    import torch
    import bench
    from cim_quantization_amd import _lib
    if not hasattr(bench, "_ALL_LAYERS"):
        bench._ALL_LAYERS = list(bench.RESNET20)
    names = [r[0] for r in bench._ALL_LAYERS]
    bench.RESNET20[:] = [bench._ALL_LAYERS[names.index(layer)]]
    layers, xs, gs = bench.build(torch.device("cuda:0"), 256)
    m, x, g = layers[0], xs[0], gs[0]
    for name in VARIANTS:
        _lib._lib = _lib.load(lib_path(name))
        x1 = x.detach().requires_grad_(True)
        m(x1).backward(g)  # warm (alpha init etc.)
        torch.cuda.synchronize()
        res = {}
        for kern in ("fwd", "bwd_gx", "bwd_gw", "prep_act"):
            with _lib.KernelTimer(kern) as kt:
                for _ in range(iters):
                    x1 = x.detach().requires_grad_(True)
                    m(x1).backward(g)
                torch.cuda.synchronize()
            res[kern] = kt.total_ms / max(kt.launches, 1) * 1000
        print(f"{layer:16s} {name:10s} " + "  ".join(f"{k}={v:8.1f}us" for k, v in res.items()), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--layer", action="append")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if a.build:
        do_build()
    else:
        for L in a.layer or ["layer1.0.conv1"]:
            do_time(L, a.iters)
