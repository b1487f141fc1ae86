"""CPU tests of the channel equalizer's host side: the NumPy restatement against the reference's recorded outputs
(tests/golden/ref_equalize.npz), the host-only entry point, the exported symbols, the C++ adapter's build and the
compat interface, and the cbf16 conversion. No GPU call is made here."""
import re
import subprocess
from pathlib import Path

import numpy as np

from tests import equalizer_ref as E

ROOT = Path(__file__).resolve().parent.parent
ADAPTERS = ROOT / "srsran_projectvtlmo_amd" / "adapters"


def test_restatement_equals_the_reference_fixture():
    """Every output bit of every case; load_fixture() checks each regenerated input against its recorded SHA-256."""
    cases, outs, inputs = E.load_fixture()
    assert len(cases) == 120
    assert {(c["alg"], c["ports"], c["layers"]) for c in cases} == set(E.TOPOLOGIES)
    assert {c["n"] for c in cases} == set(E.NOF_RES) and {c["ts"] for c in cases} == set(E.TX_SCALINGS)
    assert sum("bad_port" in c for c in cases) == len(E.TOPOLOGIES)
    for c, o, inp in zip(cases, outs, inputs):
        got = E.run(E.equalize, c, inp)
        assert o["sym"].size == 2 * c["n"] * c["layers"] and o["var"].size == c["n"] * c["layers"]
        for k in ("sym", "var"):
            assert np.array_equal(got[k], o[k]), ({a: b for a, b in c.items() if a != "sha"}, k)
    var = np.concatenate([o["var"] for o in outs]).view(np.float32)
    assert np.isfinite(var).mean() >= 0.75 and (var < 0).any() and np.isinf(var).any()


def test_supported_topologies_host_only():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    got = {(a, p, l) for a in range(3) for p in range(18) for l in range(6)
           if L.ldpc_hip_equalize_supported(a, p, l) == 1}
    assert got == set(E.TOPOLOGIES) and len(got) == 10
    assert all(L.ldpc_hip_equalize_supported(a, p, l) in (0, 1) for a in (-1, 0, 1, 2) for p in range(18)
               for l in range(6))


def test_library_exports_the_equalizer():
    from srsran_projectvtlmo_amd import _lib
    L = _lib.load()
    for name in ("ldpc_hip_equalize_supported", "ldpc_hip_equalize_launch", "ldpc_hip_equalize_sync"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    header = (ROOT / "include" / "srsran_ldpc_hip.h").read_text()
    assert "LDPC_HIP_EQ_ZF 0" in header and "LDPC_HIP_EQ_MMSE 1" in header and "} ldpc_hip_eq_desc;" in header
    assert (_lib.EQ_ZF, _lib.EQ_MMSE) == (0, 1)
    # the kernel is in the library as a gfx950 kernel of its own
    assert b"ldpc_equalize_kernel" in _lib.LIB_PATH.read_bytes()


def test_cpp_adapter_builds_and_interface_is_pure_virtual():
    subprocess.run(["make", "-C", str(ADAPTERS), "test-equalizer"], check=True, capture_output=True)
    assert (ROOT / "tests" / "cpp" / "build" / "test_equalizer").exists()
    compat = (ADAPTERS / "compat" / "srsran_minimal.h").read_text()
    m = re.search(r"class channel_equalizer\b.*?\n};", compat, re.S)
    assert m and re.search(r"virtual void equalize\(.*?\)\s*=\s*0;", m.group(0), re.S)
    f = re.search(r"class channel_equalizer_factory\b.*?\n};", compat, re.S)
    assert f and re.search(r"virtual std::unique_ptr<channel_equalizer> create\(\)\s*=\s*0;", f.group(0))


def test_to_cbf16_ties_to_even():
    from srsran_projectvtlmo_amd import equalization as eq
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)  # noqa: E731
    #            exact       tie, even kept  tie, odd up   above the tie  below the tie  carry into the exponent
    bits = [0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x3FFF8000, 0xBF808000, 0x00000000,
            0x7F800000, 0x80000000]
    want = [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x3F81, 0x4000, 0xBF80, 0x0000, 0x7F80, 0x8000]
    z = np.empty(len(bits), np.complex64)
    z.real, z.imag = f(bits), f(bits[::-1])
    got = eq.to_cbf16(z)
    assert got.dtype == np.uint16 and got.shape == (len(bits), 2)
    assert got[:, 0].tolist() == want and got[:, 1].tolist() == want[::-1]
    assert np.array_equal(got, np.stack([E.to_bf16(z.real), E.to_bf16(z.imag)], axis=-1))
    back = eq.from_cbf16(got)
    assert np.array_equal(np.ascontiguousarray(back.real).view(np.uint32) >> 16, got[:, 0])
    assert np.array_equal(eq.to_cbf16(back), got)
