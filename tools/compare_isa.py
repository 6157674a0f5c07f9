#!/usr/bin/env python3
"""Compares the device code of two builds of one csrc/*.hip file kernel by kernel (no GPU needed).

`make -C amrvolumerenderer_amd/csrc asm` writes, for every .hip source NAME.hip, its gfx950 assembly
NAME.s and the compiler's resource-usage remarks NAME.asm.log next to it.  Keep the parent's:

    make -C amrvolumerenderer_amd/csrc asm && mkdir before && cp .../csrc/*.s .../csrc/*.asm.log before   # at the parent
    make -C amrvolumerenderer_amd/csrc asm                                                               # at the head
    for s in before/*.s; do n=$(basename $s .s); \
        python tools/compare_isa.py $s .../csrc/$n.s before/$n.asm.log .../csrc/$n.asm.log | tail -1; done

Prints one line per kernel -- `identical` or the first differing instruction -- and exits non-zero
if any kernel differs, if the number of kernels differs, or if a resource figure differs.

What is normalised, and nothing else:
  * comments (`; ...`) and assembler directives (lines starting with `.`) are dropped: the
    instruction stream is the labels and instructions between a kernel's `.type NAME,@function`
    and its `.Lfunc_end`;
  * the function number in local labels (`.LBB12_3` -> `.LBB_3`), which only counts the functions
    emitted before;
  * mangled symbol names (`_Z...`) inside operands -> `SYM`.
Kernels are paired by their demangled name without the parameter types; those whose template
arguments were renamed are paired by the function name and, within it, by their order in the file,
and both names are printed so that the pairing can be read.  Resource figures: SGPRs, VGPRs,
AGPRs, both spill counts, scratch, LDS and occupancy from the -Rpass-analysis=kernel-resource-usage
remarks that `make asm` writes (the two logs).
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
from collections import defaultdict

_TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
_END = re.compile(r"^\.Lfunc_end\d+:")
_LABEL_NO = re.compile(r"\.LBB\d+_")
_SYMBOL = re.compile(r"\b_Z\w+")
_FIGURES = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
            "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def kernels_of(path):
    """[(mangled name, [normalised instruction lines])] in file order; only the functions that are
    kernels (those with an .amdhsa_kernel descriptor)."""
    functions, name, body, descriptors = [], None, [], set()
    for raw in open(path):
        m = _TYPE.match(raw)
        if m:
            name, body = m.group(1), []
            continue
        if raw.startswith("\t.amdhsa_kernel "):
            descriptors.add(raw.split()[1])
        if name is None:
            continue
        if _END.match(raw):
            functions.append((name, body))
            name = None
            continue
        line = raw.split(";", 1)[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")) or line == name + ":":
            continue
        body.append(_SYMBOL.sub("SYM", _LABEL_NO.sub(".LBB_", " ".join(line.split()))))
    return [(n, b) for n, b in functions if n in descriptors]


def remarks_of(path):
    """{mangled name: {figure: value}} from the compiler's kernel-resource-usage remarks."""
    out, current = {}, None
    for raw in open(path):
        m = re.search(r"remark: Function Name: (\S+)", raw)
        if m:
            current = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass-analysis", raw)
        if m and current is not None and m.group(1) in _FIGURES:
            current[m.group(1)] = int(m.group(2))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        text = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True,
                              check=True).stdout.split("\n")
        return dict(zip(names, text))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def base_name(demangled):
    """`void avr::(anonymous namespace)::fold_plan_kernel<true, false>(int, ...)` -> fold_plan_kernel"""
    head = re.split(r"[<(]", demangled.replace("(anonymous namespace)", "anon"), 1)[0]
    return head.split()[-1].split("::")[-1]


def short_name(demangled):
    """the demangled name without its parameter list"""
    depth = 0
    text = demangled.replace("(anonymous namespace)::", "").replace("void ", "", 1)
    for i, c in enumerate(text):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0 and not text[:i].endswith("operator"):
            return text[:i]
    return text


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("before_log", help="NAME.asm.log of `make asm` (the resource-usage remarks)")
    ap.add_argument("after_log")
    args = ap.parse_args()

    sides = []
    for path, log in ((args.before, args.before_log), (args.after, args.after_log)):
        remarks = remarks_of(log)
        kernels = [(n, b, remarks.get(n, {})) for n, b in kernels_of(path)]
        names = demangle([n for n, _, _ in kernels])
        groups = defaultdict(list)
        for n, b, f in kernels:
            groups[base_name(names[n])].append((short_name(names[n]), b, f))
        sides.append((len(kernels), groups))
    (n_before, before), (n_after, after) = sides

    bad = 0
    for base in sorted(set(before) | set(after)):
        a, b = before.get(base, []), after.get(base, [])
        if len(a) != len(b):
            print(f"{base}: {len(a)} kernels before, {len(b)} after")
            bad += 1
        # the same name on both sides first, what is left (renamed template arguments) in file order
        same = {k[0] for k in a} & {k[0] for k in b}
        a = sorted(a, key=lambda k: (k[0] not in same, k[0] if k[0] in same else ""))
        b = sorted(b, key=lambda k: (k[0] not in same, k[0] if k[0] in same else ""))
        for (name_a, body_a, fig_a), (name_b, body_b, fig_b) in zip(a, b):
            label = name_a if name_a == name_b else f"{name_a} -> {name_b}"
            verdict = "identical"
            for k, (x, y) in enumerate(zip(body_a, body_b)):
                if x != y:
                    verdict = f"DIFFERS at instruction {k}: `{x}` != `{y}`"
                    break
            else:
                if len(body_a) != len(body_b):
                    verdict = f"DIFFERS in length: {len(body_a)} != {len(body_b)} instructions"
            moved = [f"{key} {fig_a.get(key)} -> {fig_b.get(key)}" for key in _FIGURES
                     if fig_a.get(key) != fig_b.get(key)]
            if not fig_a or not fig_b:
                moved.append("no resource figures found")
            if moved:
                verdict += "; RESOURCES: " + ", ".join(moved)
            else:
                verdict += (f" ({len(body_a)} lines; sgpr {fig_a['TotalSGPRs']} vgpr {fig_a['VGPRs']}"
                            f" spills {fig_a['SGPRs Spill']}/{fig_a['VGPRs Spill']}"
                            f" scratch {fig_a['ScratchSize [bytes/lane]']}"
                            f" lds {fig_a['LDS Size [bytes/block]']}"
                            f" occupancy {fig_a['Occupancy [waves/SIMD]']})")
            bad += not verdict.startswith("identical (")
            print(f"{label}: {verdict}")
    print(f"kernels: {n_before} before, {n_after} after; {bad} differ")
    return 1 if bad or n_before != n_after else 0


if __name__ == "__main__":
    sys.exit(main())
