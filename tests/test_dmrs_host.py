"""CPU tests of the PDSCH DM-RS generator's host side: the NumPy restatement (tests/dmrs_ref.py) against the reference's
recorded outputs (tests/golden/ref_dmrs.npz), the classes the fixture must hold, the two host-only entry points against
the restatement, the descriptor's layout and the row builder, and tests/cpp/test_dmrs_descs.cpp (make_dmrs_table) built
with the two host-only units it needs under AddressSanitizer and UBSan and run as a child process. No GPU call."""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np

from tests import dmrs_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "srsran_projectvtlmo_amd" / "csrc"


def test_restatement_equals_the_reference_fixture():
    """Every bit of every case: the cbf16 grid REs and the cf32 values before the rounding; load_fixture() checks each
    regenerated weight matrix against its SHA-256."""
    cases, outs, inputs = R.load_fixture()
    assert [{a: b for a, b in c.items() if a != "sha"} for c in cases] == R.cases()
    for c, (grid, pre), w in zip(cases, outs, inputs):
        what = {a: b for a, b in c.items() if a != "sha"}
        count = int(R.case_mask(c).sum())
        assert grid.size == c["ports"] * count and pre.size == 2 * grid.size, what
        got_grid, got_pre = R.run_case(c, w)
        assert np.array_equal(got_grid, grid), what
        assert np.array_equal(got_pre, pre), what
        # the recorded cf32 values round to the recorded grid
        f = pre.view(np.float32).reshape(-1, 2)
        assert np.array_equal(R.P.to_cbf16(f[:, 0], f[:, 1]), grid), what


def test_fixture_holds_every_class():
    cases, outs, _ = R.load_fixture()
    classes = R.fixture_classes(cases, outs)
    assert len(classes) >= 17
    missing = [name for name, seen in classes.items() if not seen]
    assert not missing, f"missing from the fixture: {missing}"


def test_c_init_and_supported_host_only():
    from srsran_projectvtlmo_amd import _lib, signal_processors as sp
    L = _lib.load()
    for slot in (0, 1, 9, 19, 79, 159):
        for l in range(R.NSYMB):
            for sid in (0, 1, 41, 513, 32768, 65535):
                for n in (0, 1):
                    assert L.ldpc_hip_dmrs_pdsch_c_init(slot, l, sid, n) == R.c_init(slot, l, sid, n), (slot, l, sid, n)
    # the wrap case: the reference's 32-bit product wraps, and wrapping first gives the same value
    exact = (14 * 159 + 14) * (2 * 65535 + 1) * (1 << 17) + 2 * 65535 + 1
    assert exact >= 1 << 32 and exact % (1 << 31) == (exact % (1 << 32)) % (1 << 31)
    assert sp.dmrs_pdsch_c_init(159, 13, 65535, 1) == exact % (1 << 31)
    got = {(t, l, p) for t in range(4) for l in range(7) for p in range(7)
           if L.ldpc_hip_dmrs_pdsch_supported(t, l, p) == 1}
    assert got == {(t, l, p) for t in (1, 2) for l, p in R.TOPOLOGIES} and len(got) == 20
    assert sp.dmrs_pdsch_supported(2, 2, 4) and not sp.dmrs_pdsch_supported(1, 3, 2)
    assert not sp.dmrs_pdsch_supported(3, 1, 1)


def test_library_exports_the_generator_and_the_descriptor_layout():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    for name in ("ldpc_hip_dmrs_pdsch_supported", "ldpc_hip_dmrs_pdsch_c_init", "ldpc_hip_dmrs_pdsch_map_launch"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "srsran_ldpc_hip.h").read_text()
    m = re.search(r"typedef struct \{\s*/\* 64 bytes \*/(.*?)\} ldpc_hip_dmrs_pdsch_desc;", header, re.S)
    assert m
    # the header's fields in order, against the ctypes mirror
    names = re.findall(r"\b(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [f[0] for f in _lib.DmrsPdschDesc._fields_]
    assert ctypes.sizeof(_lib.DmrsPdschDesc) == 64
    assert _lib.DmrsPdschDesc.amplitude.offset == 52 and _lib.DmrsPdschDesc.symbols_mask.offset == 56
    assert _lib.DmrsPdschDesc.type.offset == 58 and _lib.DmrsPdschDesc.n_scid.offset == 61
    assert re.search(r"#define LDPC_HIP_SYM_CBF16\s+2\b", header) and _lib.SYM_CBF16 == 2
    # the kernel is in the library as a gfx950 kernel of its own
    assert b"ldpc_dmrs_kernel" in _lib.LIB_PATH.read_bytes()


def test_rows_builder():
    from srsran_projectvtlmo_amd import signal_processors as sp
    rows = sp.dmrs_rows()
    total = 0
    for c in R.cases():
        w = R.case_input(c)
        sym = np.zeros(R.NSYMB, bool)
        sym[c["symbols"]] = True
        cfg = sp.config_t(c["slot"], c["ref"], c["type"], c["id"], bool(c["n_scid"]), c["amplitude"], sym,
                          R.case_rb_mask(c), w)
        n = rows.add((c["grid_ports"], R.NSYMB, c["nrb"] * R.NRE), cfg, grid_offset=3 + total)
        assert n == int(R.case_mask(c).sum())
        r = rows.rows[-1]
        assert r["grid_offset"] == 3 + total and r["symbol_stride"] == r["width"] == c["nrb"] * R.NRE
        assert r["port_stride"] == R.NSYMB * r["width"] and r["nof_rb"] == c["nrb"]
        assert (r["type"], r["nof_layers"], r["nof_ports"]) == (c["type"], c["layers"], c["ports"])
        assert r["symbols_mask"] == sum(1 << l for l in c["symbols"])
        for n_rb in range(c["nrb"]):
            word = int(rows.masks[r["mask_offset"] + n_rb // 64])
            assert bool((word >> (n_rb % 64)) & 1) == bool(R.case_rb_mask(c)[n_rb])
        got = rows.weights[r["weight_offset"]:r["weight_offset"] + w.size]
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(w).reshape(-1).view(np.uint32))
        total += n
    # equal RB masks share their words
    assert rows.masks.size == sum((n + 63) // 64 for n, _ in {(c["nrb"], R.case_rb_mask(c).tobytes())
                                                               for c in R.cases()})
    arr, wf, m = rows.descriptors()
    assert wf.dtype == np.float32 and wf.size == 2 * rows.weights.size and m.dtype == np.uint64
    assert arr[1].slot_index == R.cases()[1]["slot"] and arr[1].scrambling_id == R.cases()[1]["id"]
    import pytest
    cfg.precoding = np.ones((2, 1, 1), np.complex64)
    with pytest.raises(ValueError):
        rows.add((1, R.NSYMB, 132), cfg)                                      # more than one PRG
    cfg.precoding = np.ones((2, 1), np.complex64)
    with pytest.raises(ValueError):
        rows.add((1, R.NSYMB, 132), cfg)                                      # more precoding ports than grid ports


def test_table_translation_under_sanitizers():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    build = ROOT / "tests" / "cpp" / "build"
    build.mkdir(parents=True, exist_ok=True)
    exe = build / "test_dmrs_descs"
    srcs = [ROOT / "tests" / "cpp" / "test_dmrs_descs.cpp", CSRC / "ldpc_hip_descs.cpp", CSRC / "ldpc_graph.cpp"]
    deps = srcs + sorted(CSRC.glob("*.h")) + [CSRC / "ldpc_base_graphs.inc", ROOT / "include" / "srsran_ldpc_hip.h"]
    if not exe.exists() or exe.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-D__HIP_PLATFORM_AMD__", "-include", "hip/hip_runtime_api.h", f"-I{rocm / 'include'}",
               f"-I{ROOT / 'include'}", f"-I{CSRC}", "-o", str(exe)] + [str(s) for s in srcs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
