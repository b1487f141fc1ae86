"""CPU test of the descriptor translations (csrc/ldpc_hip_descs.cpp): builds tests/cpp/test_descs.cpp with the two
host-only units it needs under AddressSanitizer and UBSan and runs it as a child process. No GPU, no HIP runtime call:
the HIP headers only supply the function attributes the shared type header uses."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "srsran_projectvtlmo_amd" / "csrc"


def test_descriptor_translations_under_sanitizers():
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    build = ROOT / "tests" / "cpp" / "build"
    build.mkdir(parents=True, exist_ok=True)
    exe = build / "test_descs"
    srcs = [ROOT / "tests" / "cpp" / "test_descs.cpp", CSRC / "ldpc_hip_descs.cpp", CSRC / "ldpc_graph.cpp"]
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
