#!/usr/bin/env python3
"""Writes tests/golden/ldpc_base_graph_shifts.json: per base-graph edge (row-major) [bg, row, col, shift for iLS 0..7],
the numbers of 3GPP TS 38.212 Tables 5.3.2-2 / 5.3.2-3 as the reference's ldpc_luts_impl.cpp holds them, extracted
and cross-checked by tools/gen_ldpc_tables.py (which reads that file as text; its path is this script's argument).
tests/test_reference_pins.py holds csrc/ldpc_base_graphs.inc to this fixture. Data only."""
import importlib.util
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
OUT = Path(__file__).resolve().parent / "ldpc_base_graph_shifts.json"


def main():
    if len(sys.argv) != 2:
        sys.exit("usage: make_base_graph_shifts.py <path of the reference's ldpc_luts_impl.cpp>")
    spec = importlib.util.spec_from_file_location("gen_ldpc_tables", ROOT / "tools" / "gen_ldpc_tables.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    text = gen.generate(Path(sys.argv[1]))
    edges = [[int(x) for x in m.split(",")] for m in re.findall(r"^LDPC_EDGE\(([^)]*)\)$", text, flags=re.M)]
    if len(edges) != 316 + 197:
        sys.exit(f"expected 513 edges, found {len(edges)}")
    OUT.write_text(json.dumps({"source": "ldpc_luts_impl.cpp (BG1_matrices, BG2_matrices)",
                               "columns": ["bg", "row", "col", "s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7"],
                               "edges": edges}, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    print(f"{len(edges)} edges -> {OUT}")


if __name__ == "__main__":
    main()
