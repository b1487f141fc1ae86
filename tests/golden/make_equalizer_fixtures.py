"""Records tests/golden/ref_equalize.npz from the reference's channel equalizer.

    python tests/golden/make_equalizer_fixtures.py [REFERENCE_TREE]

Not run by any test. Compiles a small shim of our own (below: it only includes reference headers) together with the
reference tree's channel_equalizer_generic_impl.cpp, in place, with the flags of oracle/Makefile's `ref` target
(-O2 -march=x86-64 -ffp-contract=off: SRSRAN_SIMD_CF_SIZE is 0, so only the scalar loops are built), into the
git-ignored oracle/_ref/libsrsran_ref_equalizer.so. The file holds, per case of tests/equalizer_ref.py's cases(), the
parameters with the seed, the SHA-256 of the input regenerated from the seed, and the bit patterns the reference wrote
(one record per output, equalizer_ref.pack_outputs).tests/test_equalizer_host.py holds the NumPy restatement to it,
tests/test_gpu_equalizer.py the HIP kernel."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import equalizer_ref as E  # noqa: E402
from tests.ref_cases import digest  # noqa: E402

MAX_BYTES = 106098  # as tests/golden/make_reference_fixtures.py allows
REF_FLAGS = "-std=c++17 -O2 -march=x86-64 -ffp-contract=off -fPIC -DASSERTS_ENABLED -DFMT_HEADER_ONLY -w".split()
OUT = ROOT / "oracle" / "_ref" / "libsrsran_ref_equalizer.so"

SHIM = r"""
#include "channel_equalizer_generic_impl.h"
#include "srsran/adt/tensor.h"
#include <cstring>
using namespace srsran;
static_assert(sizeof(cbf16_t) == 4, "cbf16 is two bf16");
extern "C" int ref_equalize(int algorithm, unsigned nof_re, unsigned nof_ports, unsigned nof_layers,
                            const uint16_t* ch_symbols, const uint16_t* ch_estimates, const float* noise_vars,
                            float tx_scaling, float* eq_symbols, float* eq_noise_vars)
{
  dynamic_tensor<2, cbf16_t, channel_equalizer::re_list::dims>     sym({nof_re, nof_ports});
  dynamic_tensor<3, cbf16_t, channel_equalizer::ch_est_list::dims> est({nof_re, nof_ports, nof_layers});
  std::memcpy(sym.get_data().data(), ch_symbols, sizeof(cbf16_t) * sym.get_data().size());
  std::memcpy(est.get_data().data(), ch_estimates, sizeof(cbf16_t) * est.get_data().size());
  channel_equalizer_generic_impl eq(algorithm == 0 ? channel_equalizer_algorithm_type::zf
                                                   : channel_equalizer_algorithm_type::mmse);
  eq.equalize(span<cf_t>(reinterpret_cast<cf_t*>(eq_symbols), nof_re * nof_layers),
              span<float>(eq_noise_vars, nof_re * nof_layers), sym, est, span<const float>(noise_vars, nof_ports),
              tx_scaling);
  return 0;
}
"""


def build(ref: Path) -> ctypes.CDLL:
    phy = ref / "lib" / "phy" / "upper" / "equalization"
    OUT.parent.mkdir(parents=True, exist_ok=True)
    shim = OUT.parent / "ref_equalizer_shim.cpp"
    shim.write_text(SHIM)
    inc = [f"-I{ref / 'include'}", f"-I{ref / 'external'}", f"-I{ref / 'external' / 'fmt' / 'include'}", f"-I{phy}"]
    subprocess.run(["g++", *REF_FLAGS, *inc, "-shared", "-o", str(OUT), str(shim),
                    str(phy / "channel_equalizer_generic_impl.cpp")], check=True)
    lib = ctypes.CDLL(str(OUT))
    P, U, F = ctypes.c_void_p, ctypes.c_uint, ctypes.c_float
    lib.ref_equalize.restype = ctypes.c_int
    lib.ref_equalize.argtypes = [ctypes.c_int, U, U, U, P, P, P, F, P, P]
    return lib


def reference(lib):
    def fn(alg, sym, est, noise_vars, tx_scaling):
        P, n = sym.shape[:2]
        L = est.shape[0]
        sym, est = np.ascontiguousarray(sym, np.uint16), np.ascontiguousarray(est, np.uint16)
        nv = np.ascontiguousarray(noise_vars, np.float32)
        out, var = np.empty(n * L, np.complex64), np.empty(n * L, np.float32)
        lib.ref_equalize(alg, n, P, L, sym.ctypes.data, est.ctypes.data, nv.ctypes.data, float(tx_scaling),
                         out.ctypes.data, var.ctypes.data)
        return out, var
    return fn


def main():
    # the reference tree: the argument, else oracle/Makefile's SRSRAN_REF
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_REF", "/root/reference"))
    fn = reference(build(ref))
    cases = E.cases()
    outs = []
    for c in cases:
        inp = E.case_input(c)
        c["sha"] = digest(*inp)
        outs.append(E.run(fn, c, inp))
    var = np.concatenate([o["var"] for o in outs])
    sym = np.concatenate([o["sym"] for o in outs])
    off = np.cumsum([0] + [o["var"].size for o in outs]).astype(np.int64)
    np.savez_compressed(E.GOLDEN, index=np.array(json.dumps(cases, separators=(",", ":"))), off=off,
                        out=np.concatenate([E.pack_outputs(o) for o in outs]))
    size = E.GOLDEN.stat().st_size

    # from the reference's outputs alone: most REs equalise, and every abnormal outcome is there
    v = var.view(np.float32)
    finite = np.isfinite(v)
    whole = [bool(np.all(o["var"] == 0x7F800000)) for o in outs]
    bad = ["bad_port" in c for c in cases]
    print(f"{E.GOLDEN.name}: {len(cases)} cases, {v.size} outputs, {100 * finite.mean():.1f} % finite variances, "
          f"{int((v < 0).sum())} negative, {sum(whole)} cases all abnormal, {size} bytes")
    assert finite.mean() >= 0.75, "fewer than 75 % of the outputs have a finite variance"
    assert np.all(sym.reshape(-1, 2)[~finite] == 0), "an abnormal RE's symbol is +0"
    assert np.all(v[~finite] == np.inf), "an abnormal RE's variance is +inf"
    classes = {
        "an abnormal RE next to normal ones, from its estimates": any(
            not w and not b and not np.all(np.isfinite(o["var"].view(np.float32)))
            for w, b, o in zip(whole, bad, outs)),
        "a one-layer segment all abnormal under a bad variance": any(
            w and b and c["layers"] == 1 for w, b, c in zip(whole, bad, cases)),
        "a one-layer segment that only loses a port to a bad variance": any(
            not w and b and c["layers"] == 1 for w, b, c in zip(whole, bad, cases)),
        "a two-layer segment all abnormal under a bad variance (the early return)": any(
            w and b and c["layers"] == 2 and c["n"] > 1 for w, b, c in zip(whole, bad, cases)),
        "a negative variance (two layers, negative d_pinv)": bool((v < 0).any()),
    }
    for name, seen in classes.items():
        assert seen, f"missing from the reference's outputs: {name}"
    assert size <= MAX_BYTES, f"{E.GOLDEN.name}: {size} bytes"


if __name__ == "__main__":
    main()
