"""CPU tests of the precoder's host side: the NumPy restatement against the reference's recorded outputs
(tests/golden/ref_precode.npz), the row / mask / prefix helper against a brute-force rank, the host-only entry point,
the exported symbols and the descriptor's size, and the C++ adapter's build. No GPU call is made here."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np

from tests import precoder_ref as R

ROOT = Path(__file__).resolve().parent.parent
ADAPTERS = ROOT / "srsran_projectvtlmo_amd" / "adapters"


def test_restatement_equals_the_reference_fixture():
    """Every output bit of every case, both forms; load_fixture() checks each regenerated input against its SHA-256."""
    cases, outs, inputs = R.load_fixture()
    assert [c["form"] for c in cases].count("grid") == 13 and [c["form"] for c in cases].count("compact") == 10
    for form in ("grid", "compact"):
        assert {(c["layers"], c["ports"]) for c in cases if c["form"] == form} == set(R.TOPOLOGIES)
    assert {c["qm"] for c in cases} == {2, 4, 6, 8}
    for c, o, inp in zip(cases, outs, inputs):
        what = {a: b for a, b in c.items() if a != "sha"}
        if c["form"] == "grid":
            assert o.size == c["ports"] * int(R.case_masks(c).sum())
            assert np.array_equal(R.run_grid(c, inp), o), what
        else:
            got = R.run_compact(c, inp)
            for g, w in zip(got, o):
                assert w.size == 2 * c["ports"] * c["n"] and np.array_equal(g, w), what


def test_fixture_holds_the_rounding_and_sign_cases():
    cases, outs, _ = R.load_fixture()
    by = {c["weights"]: o for c, o in zip(cases, outs) if c["form"] == "grid"}
    zero = np.concatenate([by["zero"] & 0xFFFF, by["zero"] >> 16])
    assert set(zero.tolist()) == {0x0000, 0x8000}
    tie = np.concatenate([by["tie"] & 0xFFFF, by["tie"] >> 16])
    assert set((tie & 0x7FFF).tolist()) == {0x3F80, 0x3F82}
    # a truncating conversion differs from the recorded one in about half of the components
    c, o, inp = next((c, o, i) for c, o, i in zip(*R.load_fixture()) if c["form"] == "grid" and c["layers"] == 4)
    re, im = R.map_values(R.case_masks(c), c["prg_size"], inp[1], inp[0])[2]
    trunc = (R.bits_of(re) >> 16) | (R.bits_of(im) & 0xFFFF0000)
    assert 0.2 < float((trunc.reshape(-1) != o).mean())


def test_rows_masks_and_prefix_against_a_brute_force_rank():
    from srsran_projectvtlmo_amd import precoding as pc
    for c in R.cases():
        if c["form"] != "grid":
            continue
        masks = R.case_masks(c)
        nsubc = c["nrb"] * R.NRE
        w = R.case_input(c)[1]
        rows = pc.precode_rows()
        count = rows.add((c["ports"], R.NSYMB, nsubc), masks, c["prg_size"], w, sym_offset=5, grid_offset=3)
        assert count == int(masks.sum())
        used = [l for l in range(R.NSYMB) if masks[l].any()]
        assert len(rows.rows) == len(used)
        # rows that share a mask share its words
        assert rows.masks.size == len({masks[l].tobytes() for l in used}) * ((nsubc + 63) // 64)
        assert rows.prefix.size == rows.masks.size
        seen = 0
        for r, l in zip(rows.rows, used):
            assert r["sym_offset"] == 5 + c["layers"] * seen and r["grid_offset"] == 3 + l * nsubc
            assert r["port_stride"] == R.NSYMB * nsubc and r["width"] == nsubc
            assert (r["nof_layers"], r["nof_ports"], r["nof_prg"]) == (c["layers"], c["ports"], w.shape[0])
            rank = 0
            for k in range(nsubc):  # brute force: the rank of a masked subcarrier is the masked ones below it
                word = int(rows.masks[r["mask_offset"] + k // 64])
                assert bool((word >> (k % 64)) & 1) == bool(masks[l, k])
                if masks[l, k]:
                    below = bin(word & ((1 << (k % 64)) - 1)).count("1")
                    assert int(rows.prefix[r["mask_offset"] + k // 64]) + below == rank
                    rank += 1
            last = int(rows.masks[r["mask_offset"] + (nsubc - 1) // 64])
            assert nsubc % 64 == 0 or last >> (nsubc % 64) == 0
            seen += rank
        # the weights as the launch gets them: [prg][port][layer], scaling 1
        assert np.array_equal(rows.weights.view(np.uint32), np.ascontiguousarray(w).reshape(-1).view(np.uint32))
        arr, wf, m = rows.descriptors()
        assert wf.dtype == np.float32 and wf.size == 2 * w.size and m.dtype == np.uint64
        assert arr[0].width == nsubc and arr[0].prg_size == c["prg_size"]


def test_scaling_is_applied_per_component_in_float32():
    from srsran_projectvtlmo_amd import precoding as pc
    w = R.case_input(R.cases()[4])[1]
    s = R.modulation_scaling(8)
    rows = pc.precode_rows()
    rows.add((2, 14, 300), R.case_masks(R.cases()[4]), 4, w, float(s))
    assert np.array_equal(rows.weights.view(np.uint32), R.scaled(w, s).reshape(-1).view(np.uint32))
    f = np.ascontiguousarray(w).view(np.float32) * s
    assert np.array_equal(rows.weights.view(np.float32), f.reshape(-1))


def test_supported_topologies_host_only():
    from srsran_projectvtlmo_amd import _lib, precoding as pc
    L = _lib.load()
    got = {(l, p) for l in range(7) for p in range(7) if L.ldpc_hip_precode_supported(l, p) == 1}
    assert got == set(R.TOPOLOGIES) and len(got) == 10
    assert all(L.ldpc_hip_precode_supported(l, p) in (0, 1) for l in range(7) for p in range(7))
    assert pc.precode_supported(2, 4) and not pc.precode_supported(3, 2)


def test_library_exports_the_precoder_and_the_descriptor_size():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    for name in ("ldpc_hip_precode_supported", "ldpc_hip_precode_map_launch", "ldpc_hip_precode_sync"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "srsran_ldpc_hip.h").read_text()
    m = re.search(r"typedef struct \{\s*/\* 48 bytes \*/(.*?)\} ldpc_hip_precode_desc;", header, re.S)
    assert m
    # the header's fields in order, against the ctypes mirror
    names = re.findall(r"\b(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert names == [f[0] for f in _lib.PrecodeDesc._fields_]
    assert ctypes.sizeof(_lib.PrecodeDesc) == 48
    assert _lib.PrecodeDesc.width.offset == 36 and _lib.PrecodeDesc.prg_size.offset == 40
    assert _lib.PrecodeDesc.nof_ports.offset == 43
    # the kernel is in the library as a gfx950 kernel of its own
    assert b"ldpc_precode_kernel" in _lib.LIB_PATH.read_bytes()


def test_cpp_adapter_builds_and_interface_is_pure_virtual():
    subprocess.run(["make", "-C", str(ADAPTERS), "test-precoder"], check=True, capture_output=True)
    assert (ROOT / "tests" / "cpp" / "build" / "test_precoder").exists()
    compat = (ADAPTERS / "compat" / "srsran_minimal.h").read_text()
    m = re.search(r"class channel_precoder\b.*?\n};", compat, re.S)
    assert m and re.search(r"virtual void apply_precoding\(.*?\)\s*const\s*=\s*0;", m.group(0), re.S)
    assert re.search(r"virtual void apply_layer_map_and_precoding\(.*?\)\s*const\s*=\s*0;", m.group(0), re.S)
    f = re.search(r"class channel_precoder_factory\b.*?\n};", compat, re.S)
    assert f and re.search(r"virtual std::unique_ptr<channel_precoder> create\(\)\s*=\s*0;", f.group(0))
