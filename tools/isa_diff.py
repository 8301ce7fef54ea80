#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python tools/isa_diff.py PARENT_TREE NEW_TREE [-o OUT.md] [-j N] [UNIT ...]

UNIT names a translation unit under cim_quantization_amd/csrc (default: cimq_part_fwd.hip).  Each unit of
each tree is compiled device-only with build.py's flags, unbundled and disassembled; per kernel the table
holds the resource figures of both trees (the code object's metadata notes) and whether the instruction
streams are equal once addresses, symbol names and the file-name line are dropped.  Exit status 1 if the
kernel lists differ, or any kernel's resources or stream.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
ARCH = os.environ.get("CIMQ_OFFLOAD_ARCH", "gfx950")
# cim_quantization_amd/build.py's flags
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-pass-failed",
         "-mllvm", "-amdgpu-mfma-vgpr-form"]
COLS = [("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"),
        ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count"),
        ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size")]


def device_object(tree: str, unit: str, work: str) -> str:
    src = os.path.join(tree, "cim_quantization_amd", "csrc", unit)
    bundle = os.path.join(work, unit + ".bundle.o")
    obj = os.path.join(work, unit + ".gfx.o")
    subprocess.run([HIPCC] + FLAGS + ["--cuda-device-only", "-c", "-o", bundle, src], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                    f"--targets=hip-amdgcn-amd-amdhsa--{ARCH}", f"--input={bundle}", f"--output={obj}"], check=True)
    return obj


def streams(obj: str) -> "dict[str, list[str]]":
    """kernel symbol -> its instructions, in the object's order, without addresses and symbol names"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", obj], check=True,
                         capture_output=True, text=True).stdout
    out: "dict[str, list[str]]" = {}
    cur = None
    pc = 0  # instructions left in which an s_getpc_b64's pc-relative address literals can follow
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.startswith((" ", "\t")):
            ins = re.sub(r"\s*//.*$", "", line).strip()   # the trailing address comment
            ins = re.sub(r"<[^>]*>", "<>", ins)           # branch targets' symbol + offset
            if ins.startswith("s_getpc_b64"):
                pc = 3
            elif pc and re.match(r"s_addc?_u32 \S+ \S+ 0x[0-9a-f]+$", ins.replace(",", "")):
                ins = re.sub(r"0x[0-9a-f]+$", "<pcrel>", ins)  # distance to a symbol: the kernel's place, not its code
            pc = max(0, pc - 1) if not ins.startswith("s_getpc_b64") else pc
            if ins:
                cur.append(ins)
    for ins_list in out.values():  # the alignment padding after a kernel's last instruction
        while ins_list and ins_list[-1].split()[0] in ("s_nop", "s_code_end", "..."):
            ins_list.pop()
    return out


def resources(obj: str) -> "dict[str, dict[str, int]]":
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True,
                         text=True).stdout
    out: "dict[str, dict[str, int]]" = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", "\n" + txt)[1:]:
        blk = "  - .agpr_count:" + blk
        name = re.search(r"^\s*\.symbol:\s*(\S+)\.kd\s*$", blk, re.M).group(1)
        out[name] = {c: int(re.search(rf"{re.escape(k)}:\s*(\d+)", blk).group(1)) for c, k in COLS}
    return out


def occupancy(r: "dict[str, int]") -> int:
    """waves per SIMD of a gfx950 kernel: 512 unified registers in granules of 8, at most 8 waves"""
    tot = (r["vgpr"] + 7) // 8 * 8 + ((r["agpr"] + 7) // 8 * 8 if r["agpr"] else 0)
    return max(1, min(8, 512 // max(tot, 8)))


def demangle(names: "list[str]") -> "list[str]":
    try:
        d = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    except OSError:
        return names
    return d if len(d) == len(names) else names


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("units", nargs="*", default=["cimq_part_fwd.hip"])
    ap.add_argument("-o", "--out", default=None, help="the table (markdown); default: standard output")
    ap.add_argument("-j", "--jobs", type=int, default=4)
    a = ap.parse_intermixed_args()
    bad = 0
    rows = ["| unit | kernel | " + " | ".join(f"{c} parent / new" for c, _ in COLS) +
            " | occupancy parent / new | instructions parent / new | stream |", "|" + "---|" * (len(COLS) + 5)]
    with tempfile.TemporaryDirectory() as work:
        jobs = {}
        with concurrent.futures.ThreadPoolExecutor(max(1, a.jobs)) as ex:
            for u in a.units:
                for side, tree in (("parent", a.parent), ("new", a.new)):
                    d = os.path.join(work, side)
                    os.makedirs(d, exist_ok=True)
                    jobs[u, side] = ex.submit(device_object, tree, u, d)
        for u in a.units:
            po, no = jobs[u, "parent"].result(), jobs[u, "new"].result()
            ps, ns, pr, nr = streams(po), streams(no), resources(po), resources(no)
            pk, nk = [k for k in ps if k in pr], [k for k in ns if k in nr]
            if pk != nk:
                bad += 1
                rows.append(f"| {u} | kernel lists differ: {len(pk)} parent, {len(nk)} new | " + " | " * (len(COLS) + 2) + "|")
            for k, dn in zip(nk, demangle(nk)):
                if k not in pr:
                    continue
                eq = ps[k] == ns[k]
                same = eq and pr[k] == nr[k]
                bad += 0 if same else 1
                dn = re.sub(r"^void |\((?:[^()]|\([^()]*\))*\)$", "", dn)  # the name without its parameter list
                dn = dn.replace("cimq::", "").replace("|", "\\|")
                rows.append(f"| {u} | `{dn}` | " + " | ".join(f"{pr[k][c]} / {nr[k][c]}" for c, _ in COLS) +
                            f" | {occupancy(pr[k])} / {occupancy(nr[k])} | {len(ps[k])} / {len(ns[k])} | "
                            f"{'equal' if eq else 'DIFFERS'} |")
    text = "\n".join(rows) + f"\n\n{bad} difference(s)\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
        print(f"{bad} difference(s); table in {a.out}")
    else:
        sys.stdout.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
