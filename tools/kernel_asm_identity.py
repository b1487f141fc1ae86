#!/usr/bin/env python3
"""CPU only: compare the gfx950 assembly of two source trees kernel by kernel (a refactor's "device code unchanged").

  python tools/kernel_asm_identity.py OLD_CSRC NEW_CSRC [--multiset] [--keep DIR [--reuse]] [-j N]

Every kernel unit of each tree is compiled as `make -n -B` in its csrc directory would compile it (the product flags),
with `--cuda-device-only -S` instead of `-c`, and the assembly is cut into kernels by symbol, so a kernel may move
between units. Reported: the kernel count per side, the names only one side has, and every kernel whose text differs.
Basic-block labels carry the function's number within its unit (.LBB12_3, and BB12_3 in the loop comments): the
number is dropped and runs of blanks are collapsed; nothing else is normalised.

--multiset: for kernels whose text differs, also say whether the resource figures of the kernel's descriptor comments
(SGPRs, VGPRs, AGPRs, scratch, LDS, occupancy) and the sorted instruction lines are equal (a reordering only).
Exit status 0 when every kernel is identical (with --multiset: a reordering with equal figures at most).
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FIGURES = ("NumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def unit_commands(csrc):
    """(name, argv) per .hip unit: the Makefile's own compile line, emitting device assembly"""
    out = subprocess.run(["make", "-n", "-B", "-C", csrc], check=True, capture_output=True, text=True).stdout
    cmds = []
    for line in out.splitlines():
        w = line.split()
        if "-c" not in w or not w[-1].endswith(".hip"):
            continue
        obj = w[w.index("-o") + 1]
        w[w.index("-c")] = "--cuda-device-only"
        w.insert(w.index("-o"), "-S")
        cmds.append((os.path.basename(obj)[:-2], w))
    return cmds


def compile_units(csrc, outdir, jobs, reuse):
    os.makedirs(outdir, exist_ok=True)
    files = []

    def one(item):
        name, w = item
        path = os.path.join(outdir, name + ".s")
        w = list(w)
        w[w.index("-o") + 1] = path
        if not (reuse and os.path.exists(path)):
            subprocess.run(w, check=True, cwd=csrc, capture_output=True)
        return path

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        files = list(ex.map(one, unit_commands(csrc)))
    return files


def kernels_of(path):
    """kernel name -> its lines from the entry label to the end of its descriptor comments"""
    text = open(path).read().splitlines()
    names = {m.group(1) for l in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out, cur, last = {}, None, None
    fig = re.compile(r";\s*(%s):\s*\d+" % "|".join(FIGURES))
    for l in text:
        m = re.match(r"(\S+):\s*(;.*)?$", l)
        if cur is None and m and m.group(1) in names:
            cur = last = m.group(1)
            out[cur] = []
            continue
        if cur is None and last is not None and fig.match(l.strip()):
            out[last].append(" ".join(l.split()))  # the resource comments that follow the kernel's code
        if cur is not None:
            if l.startswith("\t.section") and ".AMDGPU.csdata" not in l and out[cur]:
                cur = None
                continue
            s = re.sub(r"\.L(BB|tmp|func_end|func_begin)\d+", r".L\1", " ".join(l.split()))
            s = re.sub(r"\bBB\d+_", "BB_", s)  # the same number in the loop comments
            if s and not s.startswith((".p2align", ".section", ".text")):
                out[cur].append(s)
    return out


def figures(lines):
    f = {}
    for l in lines:
        m = re.match(r";\s*(\w+):\s*(\d+)", l)
        if m and m.group(1) in FIGURES:
            f[m.group(1)] = int(m.group(2))
    return f


def instructions(lines):
    return sorted(l.split(";")[0].strip() for l in lines if l and l[0] not in ";." and not l.endswith(":"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--multiset", action="store_true")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    ap.add_argument("--reuse", action="store_true", help="with --keep: do not recompile a unit whose .s is there")
    ap.add_argument("-j", type=int, default=16)
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="kasm_")
    side = {}
    for tag, csrc in (("old", a.old), ("new", a.new)):
        ks = {}
        for f in compile_units(csrc, os.path.join(tmp, tag), a.j, a.reuse):
            for k, v in kernels_of(f).items():
                if k in ks:
                    sys.exit(f"{tag}: kernel {k} defined in two units")
                ks[k] = v
        side[tag] = ks
        print(f"{tag}: {csrc}: {len(ks)} kernels")
    old, new = side["old"], side["new"]
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    print(f"names only in old: {only_old if only_old else 'none'}")
    print(f"names only in new: {only_new if only_new else 'none'}")
    differ, bad = [], 0
    for k in sorted(set(old) & set(new)):
        if old[k] != new[k]:
            differ.append(k)
    print(f"kernels in both: {len(set(old) & set(new))}, identical text: {len(set(old) & set(new)) - len(differ)}, "
          f"different: {len(differ)}")
    for k in differ:
        if not a.multiset:
            print(f"  DIFFERENT {k}")
            bad += 1
            continue
        fo, fn = figures(old[k]), figures(new[k])
        same_f, same_i = fo == fn, instructions(old[k]) == instructions(new[k])
        bad += 0 if (same_f and same_i) else 1
        print(f"  {k}: figures {'equal' if same_f else f'{fo} -> {fn}'}; instruction multiset "
              f"{'equal (reordered)' if same_i else f'DIFFERENT ({len(instructions(old[k]))} -> {len(instructions(new[k]))})'}")
    return 1 if (bad or only_old or only_new) else 0


if __name__ == "__main__":
    sys.exit(main())
