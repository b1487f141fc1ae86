"""Runs the C++ precoder test program (tests/cpp/test_precoder.cpp): precoders made by
create_channel_precoder_factory_hip run both channel_precoder methods for all ten topologies against the scalar rule
the program carries."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
ADAPTERS = ROOT / "srsran_projectvtlmo_amd" / "adapters"
PROGRAM = ROOT / "tests" / "cpp" / "build" / "test_precoder"


@pytest.mark.gpu
def test_cpp_precoder_all_topologies():
    subprocess.run(["make", "-s", "-C", str(ADAPTERS), "test-precoder"], check=True)
    r = subprocess.run([str(PROGRAM)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
