"""CPU tests of the PUSCH DM-RS channel estimator's host side: the NumPy restatement (tests/chest_ref.py) against the
reference's recorded outputs (tests/golden/ref_chest.npz), the classes the fixture must hold, the C finalizer against the
recorded metrics, the struct layouts, the row builder, and tests/cpp/test_chest_descs.cpp (make_chest_table,
chest_filter, chest_finalize) built with the two host-only units it needs under AddressSanitizer and UBSan and run as a
child process. No GPU call."""
import ctypes
import functools
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import chest_ref as R

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "srsran_projectvtlmo_amd" / "csrc"


@functools.lru_cache(maxsize=1)
def _fixture():
    return R.load_fixture()


@functools.lru_cache(maxsize=1)
def _restated():
    cases, _, grids = _fixture()
    return [R.run_case(c, g) for c, g in zip(cases, grids)]


def _what(c):
    return {a: b for a, b in c.items() if a != "sha"}


def test_restatement_equals_the_reference_fixture():
    """Every bit of every plane of every case: filtered pilots, interpolated cf32 values, cbf16 estimates and the five
    metrics; load_fixture() checks each regenerated grid against its SHA-256."""
    cases, outs, _ = _fixture()
    assert [_what(c) for c in cases] == R.cases()
    for c, planes, got in zip(cases, outs, _restated()):
        assert len(planes) == len(got) == c["layers"] * c["ports"]
        for i, (rec, g) in enumerate(zip(planes, got)):
            s = R.split_record(R.plane_record(g), rec["filtered"].shape[0])
            for name in ("filtered", "interp", "cbf16", "sums"):
                assert np.array_equal(s[name], rec[name]), (name, i, _what(c))
            a, b = s["metrics"].view(np.float32), rec["metrics"].view(np.float32)
            assert np.array_equal(s["metrics"][:4], rec["metrics"][:4]), (i, a, b, _what(c))
            assert s["metrics"][4] == rec["metrics"][4] or (np.isnan(a[4]) and np.isnan(b[4])), (i, a, b, _what(c))
            assert np.isnan(b[4]) == (len(c["symbols"]) == 1)
            # the recorded cf32 values round to the recorded cbf16 (bf16.h:38-55, round to nearest even)
            f = rec["interp"].view(np.float32)
            assert np.array_equal(R.P.to_cbf16(f[:, 0], f[:, 1]), rec["cbf16"])


def test_fixture_holds_every_class():
    cases, outs, grids = _fixture()
    classes = R.fixture_classes(cases)
    assert len(classes) >= 20
    missing = [name for name, seen in classes.items() if not seen]
    assert not missing, f"missing from the fixture: {missing}"
    # the unwrap branch: a jump of more than pi between the arguments of two edge pilots of the LS estimates
    wraps = 0
    for c, g in zip(cases, grids):
        if c["kind"] == "wrap" and c["strategy"] == R.FILTER:
            r = R.run_case(dict(c, strategy=R.NONE), g)[0]
            nv = R.nof_virtual_pilots(6)
            for sl in (slice(0, nv), slice(-nv, None)):
                arg = np.arctan2(r["filtered"][1][sl].astype(np.float64), r["filtered"][0][sl].astype(np.float64))
                wraps += int(np.any(np.abs(np.diff(arg)) > np.pi))
    assert wraps == 2, "the wrap case must take the unwrap branch at both ends"
    # the plane of all-zero received REs: what the reference's arg(0) path gives is pinned: a CFO of 0, a noise variance
    # of 0 (the floor is 0 too), the SNR's 1000, and estimates of +0
    seen = 0
    for c, planes in zip(cases, outs):
        if c["kind"] == "zero_port":
            m = planes[1]["metrics"].view(np.float32)
            assert m.tolist() == [0.0, 0.0, 0.0, 1000.0, 0.0] and np.all(planes[1]["cbf16"] == 0)
            assert np.all(planes[1]["interp"] == 0) and planes[0]["metrics"].view(np.float32)[1] > 0.1
            seen += 1
    assert seen == 2


def test_noise_variance_is_above_its_floor():
    """Except where the reference's estimate is zero by construction: the all-zero plane, and smoothing `none` with one
    DM-RS symbol, where the prediction from the unsmoothed LS estimate is the received pilot itself up to rounding."""
    cases, outs, _ = _fixture()
    for c, planes in zip(cases, outs):
        for i, rec in enumerate(planes):
            m = rec["metrics"].view(np.float32)
            if c["kind"] == "zero_port" and i == 1:
                continue
            if c["strategy"] == R.NONE and len(c["symbols"]) == 1:
                assert m[2] == np.float32(m[1] / np.float32(1e10))
                continue
            assert m[2] > 100.0 * m[1] / 1e10, (i, m, _what(c))


def test_float64_mode_is_close_to_float32():
    """The two modes of the restatement agree to float32 precision over the band (the recurrence carries its rounding
    on, so the bound grows with the pilots)."""
    cases, _, grids = _fixture()
    for c, g, r32 in zip(cases, grids, _restated()):
        if sum(e - b for b, e in c["rbs"]) > 43:
            continue
        for a, b in zip(r32, R.run_case(c, g, np.float64)):
            top = max(np.abs(b["interp"][0]).max(), np.abs(b["interp"][1]).max(), 1e-30)
            for k in (0, 1):
                assert np.abs(a["interp"][k] - b["interp"][k]).max() <= 2.0 ** -17 * top, _what(c)
            if top > 1e-20:
                assert np.allclose(a["metrics"][:4], b["metrics"][:4], rtol=1e-4), _what(c)


def test_finalizer_equals_the_recorded_metrics():
    """ldpc_hip_dmrs_pusch_finalize on the file's own raw sums gives the file's epre, rsrp, noise variance, snr and
    cfo_Hz bit for bit."""
    from srsran_projectvtlmo_amd import signal_processors as sp
    cases, outs, _ = _fixture()
    for c, planes in zip(cases, outs):
        sym = np.zeros(R.NSYMB, bool)
        sym[c["symbols"]] = True
        n = R.DPR * int(R.case_rb_mask(c).sum())
        recs = np.zeros((len(planes), 8), np.uint32)
        for i, rec in enumerate(planes):
            recs[i, :5] = rec["sums"]
            recs[i, 5] = n
        got = sp.chest_results(recs, c["scaling"], sym, c["numerology"])
        for rec, g in zip(planes, got):
            want = rec["metrics"].view(np.float32)
            have = np.array([g["epre"], g["rsrp"], g["noise_var"], g["snr"]], np.float32)
            assert np.array_equal(have.view(np.uint32), rec["metrics"][:4]), (have, want, _what(c))
            if len(c["symbols"]) == 1:
                assert g["cfo_Hz"] is None and np.isnan(want[4])
            else:
                assert np.float32(g["cfo_Hz"]).view(np.uint32) == rec["metrics"][4], (g["cfo_Hz"], want[4], _what(c))


def test_midpoint_share_is_below_one_percent():
    """Where the device's `filter` deviation may move a cbf16 rounding: the share of the file's cf32 components within
    the bound of a midpoint between two bf16 values, per `filter` case, from the file alone."""
    assert R.FILTER_BOUND <= 2.0 ** -16
    cases, outs, _ = _fixture()
    for c, planes in zip(cases, outs):
        if c["strategy"] == R.FILTER:
            sizes = [rec["interp"].size for rec in planes]
            share = sum(R.midpoint_share(rec["interp"], R.FILTER_BOUND) * n for rec, n in zip(planes, sizes)) / sum(sizes)
            assert share < 0.01, (share, _what(c))


def test_library_exports_the_estimator_and_the_struct_layouts():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    for name in ("ldpc_hip_dmrs_pusch_supported", "ldpc_hip_dmrs_pusch_estimate_launch",
                 "ldpc_hip_dmrs_pusch_finalize"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "srsran_ldpc_hip.h").read_text()
    for size, cname, mirror in ((104, "ldpc_hip_dmrs_pusch_desc", _lib.DmrsPuschDesc),
                                (32, "ldpc_hip_chest_result", _lib.ChestResult),
                                (24, "ldpc_hip_chest_metrics", _lib.ChestMetrics)):
        m = re.search(r"typedef struct \{\s*/\* %d bytes \*/([^}]*?)\} %s;" % (size, cname), header, re.S)
        assert m, cname
        # the header's fields in order, against the ctypes mirror
        names = re.findall(r"\b(\w+)(?:\[\d+\])?[,;]", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
        assert names == [f[0] for f in mirror._fields_], cname
        assert ctypes.sizeof(mirror) == size
    D = _lib.DmrsPuschDesc
    assert D.pilots_offset.offset == 48 and D.result_offset.offset == 56 and D.scaling.offset == 84
    assert D.symbols_mask.offset == 88 and D.type.offset == 90 and D.strategy.offset == 96 and D.rx_ports.offset == 98
    assert _lib.ChestResult.nof_pilots.offset == 20 and _lib.ChestMetrics.has_cfo.offset == 20
    assert re.search(r"#define LDPC_HIP_CHEST_NONE\s+0\b", header) and _lib.CHEST_NONE == 0
    assert re.search(r"#define LDPC_HIP_CHEST_FILTER\s+1\b", header) and _lib.CHEST_FILTER == 1
    # the kernel is in the library as a gfx950 kernel of its own
    assert b"ldpc_chest_kernel" in _lib.LIB_PATH.read_bytes()
    got = {(t, l, p, s, k) for t in range(4) for l in range(6) for p in range(6) for s in range(4) for k in range(2)
           if L.ldpc_hip_dmrs_pusch_supported(t, l, p, s, k) == 1}
    assert got == {(1, l, p, s, 0) for l in range(1, 5) for p in range(1, 5) for s in (0, 1)}


def _config(sp, c):
    sym = np.zeros(R.NSYMB, bool)
    sym[c["symbols"]] = True
    return sp.pusch_config_t(c["slot"], c["numerology"], 1, c["id"], bool(c["n_scid"]), c["scaling"], sym,
                             R.case_rb_mask(c), c["first"], c["nsymb"], c["layers"], c["rx_ports"])


def test_rows_builder_and_what_is_not_implemented():
    from srsran_projectvtlmo_amd import signal_processors as sp
    rows = sp.chest_rows()
    for i, c in enumerate(R.cases()):
        nsubc = c["nrb"] * R.NRE
        n = rows.add((c["grid_ports"], R.NSYMB, nsubc), (c["layers"], c["ports"], R.NSYMB, nsubc), _config(sp, c),
                     "filter" if c["strategy"] == R.FILTER else "none", grid_offset=3 + i, est_offset=5 + i,
                     result_offset=7 * i, pilots_offset=11 * i)
        assert n == c["layers"] * c["ports"]
        r = rows.rows[-1]
        assert r["grid_offset"] == 3 + i and r["est_offset"] == 5 + i and r["result_offset"] == 7 * i
        assert r["grid_symbol_stride"] == r["symbol_stride"] == r["width"] == nsubc and r["nof_rb"] == c["nrb"]
        assert r["grid_port_stride"] == r["plane_stride"] == R.NSYMB * nsubc and r["pilots_offset"] == 11 * i
        assert (r["nof_layers"], r["nof_rx_ports"], r["strategy"]) == (c["layers"], c["ports"], c["strategy"])
        assert r["symbols_mask"] == sum(1 << l for l in c["symbols"]) and r["rx_ports"][:c["ports"]] == tuple(c["rx_ports"])
        assert (r["first_symbol"], r["nof_symbols"], r["grid_ports"]) == (c["first"], c["nsymb"], c["grid_ports"])
        for n_rb in range(c["nrb"]):
            word = int(rows.masks[r["mask_offset"] + n_rb // 64])
            assert bool((word >> (n_rb % 64)) & 1) == bool(R.case_rb_mask(c)[n_rb])
    arr, m = rows.descriptors()
    c1 = R.cases()[1]
    assert arr[1].slot_index == c1["slot"] and arr[1].scrambling_id == c1["id"] and m.dtype == np.uint64
    assert list(arr[6].rx_ports)[:2] == R.cases()[6]["rx_ports"] and abs(arr[1].scaling - c1["scaling"]) < 1e-7
    # equal RB masks share their words
    assert rows.masks.size == sum((n + 63) // 64 for n, _ in {(c["nrb"], R.case_rb_mask(c).tobytes())
                                                               for c in R.cases()})
    c = R.cases()[0]
    shape = ((1, R.NSYMB, 132), (1, 1, R.NSYMB, 132))
    cfg = _config(sp, c)
    with pytest.raises(NotImplementedError):
        sp.chest_rows().add(*shape, cfg, "mean")
    with pytest.raises(NotImplementedError):
        sp.chest_rows().add(*shape, cfg, "filter", compensate_cfo=True)
    cfg.type = sp.TYPE2
    with pytest.raises(NotImplementedError):
        sp.chest_rows().add(*shape, cfg)
    cfg = _config(sp, c)
    cfg.nof_tx_layers = 5
    with pytest.raises(NotImplementedError):
        sp.chest_rows().add(*shape, cfg)
    with pytest.raises(NotImplementedError):
        sp.create_dmrs_pusch_estimator_hip_factory("mean")
    with pytest.raises(NotImplementedError):
        sp.dmrs_pusch_estimator_hip.__init__(object.__new__(sp.dmrs_pusch_estimator_hip), "filter", True)
    cfg = _config(sp, c)
    cfg.rx_ports = [1]
    with pytest.raises(ValueError):
        sp.chest_rows().add(*shape, cfg)                                      # an rx port the grid does not have


def test_table_translation_under_sanitizers():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    build = ROOT / "tests" / "cpp" / "build"
    build.mkdir(parents=True, exist_ok=True)
    exe = build / "test_chest_descs"
    srcs = [ROOT / "tests" / "cpp" / "test_chest_descs.cpp", CSRC / "ldpc_hip_descs.cpp", CSRC / "ldpc_graph.cpp"]
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
