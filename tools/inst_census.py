#!/usr/bin/env python3
"""Static instruction census of a kernel translation unit's gfx950 assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -S --cuda-device-only gaudi_amd/csrc/<tu>.hip -o tu.s
    tools/inst_census.py tu.s [--min-loop 40] [--functions REGEX]
    tools/inst_census.py --compile kern8s_fused_192_208 [...]      (runs the hipcc line above itself)

Prints, per function and per rolled loop (a label up to the last backward branch that targets it; inner loops are counted
inside their outer loops too), how many instructions fall into each class.  The classes are general prefixes of the mnemonic --
nothing here looks for a particular instruction:

    matrix   v_mfma* / v_smfmac*                      lds      ds_*
    valu     every other v_* arithmetic               vmem     buffer_* global_* flat_*
    v_mov    v_mov* v_accvgpr* (no DPP modifier)      scratch  scratch_*
    lane     v_readlane* v_writelane* v_readfirstlane salu     s_* arithmetic, compares, moves
    dpp      any v_* carrying a DPP modifier          wait     s_waitcnt*  (of which lgkmcnt(0) alone: `drain`)
    idle     s_nop                                    barrier  s_barrier
    other    branches, scalar loads, s_setprio, s_endpgm and the like

The counts are STATIC: a loop's line says what one trip executes (if no branch inside it is taken), not how often it runs.
Weigh them with the trip counts of the shapes in question or with the SQ_INSTS_* counters
(tools/pmc_valu.sh).
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

CLASSES = ["matrix", "valu", "v_mov", "lane", "dpp", "lds", "vmem", "scratch", "salu", "wait", "idle", "barrier", "other"]
_DPP_MOD = re.compile(r"\b(quad_perm|row_shl|row_shr|row_ror|row_bcast|row_mirror|row_half_mirror|wave_shl|wave_shr|wave_rol|wave_ror|row_newbcast|dpp8):?")
_OTHER_SCALAR = ("s_branch", "s_cbranch", "s_load", "s_buffer_load", "s_endpgm", "s_setpc", "s_swappc", "s_getpc", "s_setprio",
                 "s_sleep", "s_sethalt", "s_trap", "s_code_end", "s_inst_prefetch", "s_memtime", "s_memrealtime", "s_icache", "s_call")


def classify(mnemonic: str, operands: str) -> str:
    m = mnemonic
    if m.startswith("v_"):
        if m.startswith(("v_mfma", "v_smfmac")):
            return "matrix"
        if m.endswith("_dpp") or _DPP_MOD.search(operands):
            return "dpp"
        if m.startswith(("v_readlane", "v_writelane", "v_readfirstlane")):
            return "lane"
        if m.startswith(("v_mov", "v_accvgpr")):
            return "v_mov"
        return "valu"
    if m.startswith("ds_"):
        return "lds"
    if m.startswith("scratch_"):
        return "scratch"
    if m.startswith(("buffer_", "global_", "flat_")):
        return "vmem"
    if m.startswith("s_waitcnt"):
        return "wait"
    if m == "s_nop":
        return "idle"
    if m.startswith("s_barrier"):
        return "barrier"
    if m.startswith(_OTHER_SCALAR):
        return "other"
    if m.startswith("s_"):
        return "salu"
    return "other"


_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_INST = re.compile(r"^\s+([a-z][a-z0-9_]*)\b\s*(.*?)\s*(?:;.*)?$")
_DRAIN = re.compile(r"^lgkmcnt\(0\)$")


class Function:
    def __init__(self, name: str):
        self.name = name
        self.insts: list[tuple[str, str, str]] = []  # (class, mnemonic, operands)
        self.labels: dict[str, int] = {}             # label -> index of the first instruction behind it

    def loops(self):
        """(label, first, last) per label that a later branch targets, last = the last such branch."""
        ends: dict[str, int] = {}
        for k, (cls, m, ops) in enumerate(self.insts):
            if m.startswith(("s_branch", "s_cbranch")):
                tgt = ops.split(",")[-1].strip()
                if tgt in self.labels and self.labels[tgt] <= k:
                    ends[tgt] = k
        return sorted(((lab, self.labels[lab], end) for lab, end in ends.items()), key=lambda t: t[1])


def parse(path: str) -> list[Function]:
    funcs: list[Function] = []
    cur: Function | None = None
    with open(path) as fh:
        for line in fh:
            lab = _LABEL.match(line)
            if lab:
                name = lab.group(1)
                if name.startswith(".Lfunc_end"):
                    cur = None
                elif name.startswith(".L") or name.startswith("BB"):
                    if cur is not None:
                        cur.labels[name] = len(cur.insts)
                elif not name.startswith("."):
                    cur = Function(name)
                    funcs.append(cur)
                continue
            if cur is None:
                continue
            mi = _INST.match(line)
            if not mi or line.lstrip().startswith((".", ";")):
                continue
            m, ops = mi.group(1), mi.group(2)
            cur.insts.append((classify(m, ops), m, ops))
    return [f for f in funcs if f.insts]


def count(insts) -> dict[str, int]:
    c = {k: 0 for k in CLASSES}
    c["drain"] = 0
    for cls, m, ops in insts:
        c[cls] += 1
        if cls == "wait" and _DRAIN.match(ops.strip()):
            c["drain"] += 1
    c["total"] = len(insts)
    return c


def short_name(name: str) -> str:
    try:
        out = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return name[:70]
    out = re.sub(r"\bgaudi::(w8::)?", "", out)
    cut = out.find("(")
    out = out if cut < 0 else out[:cut]
    return out if len(out) <= 70 else out[:67] + "..."


HEAD = f"{'':44s}{'total':>7s}" + "".join(f"{c:>8s}" for c in CLASSES) + f"{'drain':>7s}"


def row(title: str, c: dict[str, int]) -> str:
    return f"{title:44s}{c['total']:7d}" + "".join(f"{c[k]:8d}" for k in CLASSES) + f"{c['drain']:7d}"


def report(funcs: list[Function], min_loop: int, only: str | None, out=sys.stdout) -> None:
    pat = re.compile(only) if only else None
    for f in funcs:
        name = short_name(f.name)
        if pat and not pat.search(name) and not pat.search(f.name):
            continue
        print(f"== {name}", file=out)
        print(HEAD, file=out)
        print(row("  whole function", count(f.insts)), file=out)
        loops = f.loops()
        for lab, a, b in loops:
            if b - a + 1 < min_loop:
                continue
            depth = sum(1 for _, a2, b2 in loops if a2 <= a and b <= b2) - 1
            print(row(f"  {'  ' * min(depth, 5)}loop {lab} [{a}..{b}]"[:43], count(f.insts[a:b + 1])), file=out)
        print(file=out)


def compile_tu(tu: str, extra: list[str]) -> str:
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gaudi_amd", "csrc")
    fd, path = tempfile.mkstemp(suffix=".s", prefix=f"census_{tu}_")
    os.close(fd)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-S", "--cuda-device-only"] + extra +
                   [f"{tu}.hip", "-o", path], cwd=csrc, check=True)
    return path


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="?", help="assembly file (hipcc -S --cuda-device-only)")
    ap.add_argument("--compile", metavar="TU", help="compile gaudi_amd/csrc/TU.hip to assembly first")
    ap.add_argument("--min-loop", type=int, default=40, help="smallest loop (instructions) worth a line")
    ap.add_argument("--functions", metavar="REGEX", help="only functions whose (demangled) name matches")
    ap.add_argument("-D", action="append", default=[], help="extra -D for --compile")
    a = ap.parse_args(argv)
    if not a.asm and not a.compile:
        ap.error("an assembly file or --compile TU")
    path = a.asm
    if a.compile:
        path = compile_tu(a.compile, [f"-D{d}" for d in a.D])
    try:
        report(parse(path), a.min_loop, a.functions)
    finally:
        if a.compile:
            os.unlink(path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
