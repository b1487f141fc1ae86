#!/usr/bin/env python3
"""Diagnostic (not product): per-step instruction histogram of the specialised BG1 Z=384 decoder's iteration
(ldpc_decode_kernel<true, 0>), from its gfx950 assembly. The kernel body is split at s_barrier; the full iteration
loop is the first run of 32 step segments after the prologue. Per step: the instructions of both roles (a wave runs
one of them; split steps have one role), split into full-rate VALU, packed (v_pk_*), SALU, LDS and other, with
the VALU cost estimate of tools/asm_cost.py (cycles per wave-instruction issue).

After the steps, per iteration: the cycle-weighted issue cost by class (tools/ubench/README.md: 2.1 full rate, 2.6
full rate with a 32-bit literal, 4.25 half rate, 8.3 quarter rate; one cycle per s_nop) and the glue categories: what
the loop issues besides the packed min-sum arithmetic (pack, splat, fold, copy, select, address literals), the scalar
loads of the loop (a counted lgkmcnt wait is only safe when there are none) and the waits.

usage: python tools/step_isa.py [extra hipcc -D flags]
       python tools/step_isa.py --asm FILE.s     (the device assembly of ldpc_hip_kernels.hip compiled beforehand, as
                                                  tools/kernel_asm_identity.py OLD NEW --keep DIR leaves it in
                                                  DIR/old/ldpc_hip_kernels.s and DIR/new/ldpc_hip_kernels.s: how a
                                                  parent tree is counted without checking it out over this one)"""
import collections
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import asm_cost  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "srsran_projectvtlmo_amd" / "csrc"
LIT = re.compile(r"0x[0-9a-f]{3,}")
LABEL = re.compile(r"^([.\w$]+):")


def glue(op, line):
    """The glue category of an instruction of the iteration loop (None: not listed)."""
    if op.startswith("v_pk_"):
        return "v_pk_* (the arithmetic)"
    if op.startswith("v_perm_b32"):
        return "v_perm_b32 (pack, splat)"
    if "_sdwa" in op:
        return "SDWA forms"
    if op.startswith(("v_mad_u32_u24", "v_min3_u16", "v_max3_u16", "v_mul_u32_u24")):
        return "v_mad_u32_u24 / v_mul_u32_u24 / v_min3_u16"
    if op.startswith(("v_cmp", "v_cndmask")):
        return "v_cmp_* + v_cndmask"
    if op.startswith(("v_and_b32", "v_lshrrev_b32", "v_lshlrev_b32", "v_bfe_u32")):
        return "v_and_b32 / v_lshrrev_b32 / v_lshlrev_b32 / v_bfe_u32"
    if op.startswith("v_or_b32"):
        return "v_or_b32"
    if op.startswith("v_mov_b32"):
        return "v_mov_b32"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("v_add_u32") and LIT.search(line):
        return "v_add_u32 with a 32-bit literal"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar loads"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("ds_read_i8_d16"):
        return "ds_read_i8_d16 / _d16_hi"
    if op.startswith("ds_read"):
        return "ds_read (other)"
    if op.startswith("ds_write"):
        return "ds_write"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("v_"):
        return "other VALU"
    return None


def main():
    out = "/tmp/step_isa.s"
    if len(sys.argv) == 3 and sys.argv[1] == "--asm":
        out = sys.argv[2]
        print(f"# python tools/step_isa.py --asm {Path(out).name}")
    else:
        print("# python tools/step_isa.py " + " ".join(sys.argv[1:]))
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", f"-I{ROOT / 'include'}",
                        f"-I{CSRC}", "-mllvm", "-simplifycfg-sink-common=false", "--cuda-device-only", "-S", "-o", out,
                        str(CSRC / "ldpc_hip_kernels.hip")] + sys.argv[1:], check=True, stderr=subprocess.DEVNULL)
    src = open(out).read().split("\n")
    pat = "_ZN8ldpc_hip18ldpc_decode_kernelILb1ELi0EEEv"
    start = next(i for i, l in enumerate(src) if l.startswith(pat))
    end = start
    while not src[end].startswith(".Lfunc_end"):
        end += 1
    # instructions only; a label that heads a loop ("; =>This Loop Header" in its comment) is remembered by the index of
    # the instruction after it: the iteration loop's header bounds step 0
    header = {}
    lines = []
    for raw in src[start + 1:end]:
        l = raw.strip()
        if not l or l.startswith(";"):
            continue
        m = LABEL.match(l)
        if m:
            if "Loop Header" in l:
                header[m.group(1)] = len(lines)
            continue
        if l.startswith("."):  # assembler directive
            continue
        lines.append(l)
    bars = [i for i, l in enumerate(lines) if l.startswith("s_barrier")]
    print(f"{len(lines)} instructions, {len(bars)} barriers in ldpc_decode_kernel<true, 0> (BG1 Z=384)")
    print("step insts  valu  pk  salu  lds  other  valu_cycles~  (both roles of a step; step 0 starts at the iteration "
          "loop's header: the once-per-codeblock setup before it is not counted)")
    tot = collections.Counter()
    cls_n = collections.Counter()
    glue_n = collections.Counter()
    glue_cyc = collections.Counter()
    nops = 0
    segs = list(zip(bars, bars[1:]))
    # the full iteration loop starts at the first step holding a split row's partner merge (v_permlane32_swap): step 0
    first = next(k for k, (a, b) in enumerate(segs) if any(l.startswith("v_permlane32_swap") for l in lines[a + 1:b]))
    # step 0's segment also holds the once-per-codeblock setup: the loop starts at the last loop header inside it
    a0, b0 = segs[first]
    h0, _ = max((i, n) for n, i in header.items() if a0 < i <= b0)
    loop = [(h0 - 1, b0)] + segs[first + 1:first + 32]
    for k, (a, b) in enumerate(loop):
        seg = lines[a + 1:b]
        c = collections.Counter()
        cyc = 0.0
        for l in seg:
            op = l.split()[0]
            cls = asm_cost.classify(op, l)
            cost = asm_cost.COST.get(cls, 0)
            cyc += cost
            kind = ("lds" if op.startswith("ds_") else "salu" if op.startswith("s_") else "pk" if op.startswith("v_pk")
                    else "valu" if op.startswith("v_") else "other")
            c[kind] += 1
            cls_n[cls] += 1
            if op.startswith("s_nop"):  # s_nop N holds the issue port N + 1 cycles
                cost = int(l.split()[1], 0) + 1
                nops += cost
            g = glue(op, l)
            if g is not None:
                glue_n[g] += 1
                glue_cyc[g] += cost
        tot.update(c)
        print(f"{k:3d} {len(seg):6d} {c['valu']:5d} {c['pk']:3d} {c['salu']:5d} {c['lds']:4d} {c['other']:6d} {cyc:12.0f}")
    print("total", dict(tot))
    print()
    print("per iteration, cycle-weighted VALU issue cost by class (both roles of every step):")
    weighted = 0.0
    for cls in ("full", "full_lit", "half", "quarter"):
        w = asm_cost.COST[cls] * cls_n[cls]
        weighted += w
        print(f"  {cls:9s} {cls_n[cls]:6d} x {asm_cost.COST[cls]:4.2f} = {w:8.0f}")
    print(f"  {'s_nop':9s} {glue_n['s_nop']:6d} instructions   = {nops:8.0f}")
    print(f"  weighted issue cost {weighted + nops:.0f} cycles ({weighted:.0f} VALU + {nops} s_nop)")
    print()
    print("glue categories (count, ~issue cycles):")
    for g, n in sorted(glue_n.items(), key=lambda kv: -glue_cyc[kv[0]]):
        print(f"  {g:55s} {n:6d} {glue_cyc[g]:8.0f}")


if __name__ == "__main__":
    main()
