"""Records tests/golden/ref_dmrs.npz from the reference's PDSCH DM-RS processor.

    python tests/golden/make_dmrs_fixtures.py [REFERENCE_TREE]

Not run by any test. Compiles a small shim of our own (below: it only includes reference headers) together with the
reference tree's dmrs_pdsch_processor_impl.cpp, pseudo_random_generator_impl.cpp, resource_grid_mapper_impl.cpp,
resource_grid_writer_impl.cpp, re_pattern.cpp, channel_precoder_generic.cpp, channel_precoder_impl.cpp,
srsvec/conversion.cpp and srsvec/sc_prod.cpp, in place, with the flags of oracle/Makefile's `ref` target
(-O2 -march=x86-64 -ffp-contract=off: only the scalar loops are built), into the git-ignored
oracle/_ref/libsrsran_ref_dmrs.so. The file holds, per case of tests/dmrs_ref.py's cases(), the parameters with the
seed, the SHA-256 of the weights regenerated from the seed, and the bit patterns the reference wrote: the cbf16 DM-RS
REs of the first P ports (the rest of the grid must still hold the guard pattern), and the cf32 values before the
rounding. The latter come from a resource_grid_mapper of the shim's that stands in front of the reference's: it sees the
re_buffer_reader the processor hands over, runs the reference's channel_precoder_generic::apply_precoding on it (or,
where the reference's mapper bypasses the precoder, takes it as it is) and passes the call on.
tests/test_dmrs_host.py holds the NumPy restatement to it, tests/test_gpu_dmrs.py the HIP kernel."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import dmrs_ref as R  # noqa: E402
from tests.ref_cases import digest  # noqa: E402

MAX_BYTES = 106098  # as tests/golden/make_reference_fixtures.py allows
REF_FLAGS = "-std=c++17 -O2 -march=x86-64 -ffp-contract=off -fPIC -DASSERTS_ENABLED -DFMT_HEADER_ONLY -w".split()
OUT = ROOT / "oracle" / "_ref" / "libsrsran_ref_dmrs.so"

SHIM = r"""
#include "channel_precoder_generic.h"
#include "dmrs_pdsch_processor_impl.h"
#include "pseudo_random_generator_impl.h"
#include "resource_grid_mapper_impl.h"
#include "resource_grid_writer_impl.h"
#include "srsran/adt/tensor.h"
#include "srsran/phy/support/precoding_configuration.h"
#include "srsran/phy/support/re_pattern.h"
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>
using namespace srsran;
static_assert(sizeof(cbf16_t) == 4, "cbf16 is two bf16");

namespace {
// passes every call on to the reference's mapper; of a re_buffer_reader call it keeps the cf32 values of every port
class capture_mapper : public resource_grid_mapper
{
public:
  capture_mapper(resource_grid_mapper& next_) : next(next_) {}
  void map(const re_buffer_reader& input, const re_pattern& pattern, const precoding_configuration& precoding) override
  {
    unsigned nof_re = input.get_nof_re(), P = precoding.get_nof_ports(), L = precoding.get_nof_layers();
    if (precoding.get_nof_prg() != 1) {
      bad = true;
    }
    dynamic_re_buffer out(P, nof_re);
    out.resize(P, nof_re);
    if (L == 1 && P == 1 && precoding.get_nof_prg() == 1 && precoding.get_coefficient(0, 0, 0) == 1.0F) {
      std::memcpy(out.get_slice(0).data(), input.get_slice(0).data(), sizeof(cf_t) * nof_re);
    } else {
      precoder.apply_precoding(out, input, precoding.get_prg_coefficients(0));
    }
    sizes.push_back(P * nof_re);
    for (unsigned p = 0; p != P; ++p) {
      span<const cf_t> s = out.get_slice(p);
      for (const cf_t& v : s) {
        values.push_back(v.real());
        values.push_back(v.imag());
      }
    }
    next.map(input, pattern, precoding);
  }
  void map(symbol_buffer& buffer, const re_pattern_list& pattern, const re_pattern_list& reserved,
           const precoding_configuration& precoding, unsigned re_skip) override
  {
    next.map(buffer, pattern, reserved, precoding, re_skip);
  }
  resource_grid_mapper&   next;
  channel_precoder_generic precoder;
  std::vector<float>      values;
  std::vector<unsigned>   sizes;
  bool                    bad = false;
};
} // namespace

// grid: [port][symbol][subcarrier] cbf16, read and written; weights [port][layer]; rb: nof_rb flags; captured: per
// mapper call (one per CDM group) the cf32 values [port][symbol-major RE] as float pairs, at most cap floats
extern "C" int ref_dmrs(unsigned grid_ports, unsigned nof_rb, unsigned type, unsigned L, unsigned P,
                        const float* weights, unsigned slot_index, unsigned ref_rb, unsigned scrambling_id,
                        unsigned n_scid, float amplitude, unsigned symbols, const uint8_t* rb, uint32_t* grid,
                        float* captured, unsigned cap, unsigned* nof_calls)
{
  const unsigned nof_subc = nof_rb * NRE;
  dynamic_tensor<3, cbf16_t, resource_grid_dimensions> data({nof_subc, MAX_NSYMB_PER_SLOT, grid_ports});
  std::memcpy(data.get_data().data(), grid, sizeof(cbf16_t) * data.get_data().size());
  std::atomic<unsigned>     empty{~0U};
  resource_grid_writer_impl writer(data, empty);
  resource_grid_mapper_impl mapper(grid_ports, nof_subc, writer, std::make_unique<channel_precoder_generic>());
  capture_mapper            capture(mapper);

  dmrs_pdsch_processor::config_t config;
  config.slot                 = slot_point(4, 0, slot_index);
  config.reference_point_k_rb = ref_rb;
  config.type                 = type == 1 ? dmrs_type::TYPE1 : dmrs_type::TYPE2;
  config.scrambling_id        = scrambling_id;
  config.n_scid               = n_scid != 0;
  config.amplitude            = amplitude;
  config.symbols_mask         = symbol_slot_mask(MAX_NSYMB_PER_SLOT);
  for (unsigned l = 0; l != MAX_NSYMB_PER_SLOT; ++l) {
    if ((symbols >> l) & 1U) {
      config.symbols_mask.set(l);
    }
  }
  config.rb_mask = bounded_bitset<MAX_RB>(nof_rb);
  for (unsigned b = 0; b != nof_rb; ++b) {
    if (rb[b]) {
      config.rb_mask.set(b);
    }
  }
  precoding_weight_matrix m(L, P);
  for (unsigned p = 0; p != P; ++p) {
    for (unsigned l = 0; l != L; ++l) {
      m.set_coefficient(cf_t(weights[2 * (p * L + l)], weights[2 * (p * L + l) + 1]), l, p);
    }
  }
  config.precoding = precoding_configuration::make_wideband(m);

  dmrs_pdsch_processor_impl processor(std::make_unique<pseudo_random_generator_impl>());
  processor.map(capture, config);
  std::memcpy(grid, data.get_data().data(), sizeof(cbf16_t) * data.get_data().size());
  if (capture.bad || capture.values.size() > cap) {
    return -1;
  }
  std::memcpy(captured, capture.values.data(), sizeof(float) * capture.values.size());
  *nof_calls = capture.sizes.size();
  return static_cast<int>(capture.values.size());
}
"""


def build(ref: Path) -> ctypes.CDLL:
    lib = ref / "lib"
    OUT.parent.mkdir(parents=True, exist_ok=True)
    shim = OUT.parent / "ref_dmrs_shim.cpp"
    shim.write_text(SHIM)
    support, prec = lib / "phy" / "support", lib / "phy" / "generic_functions" / "precoding"
    upper = lib / "phy" / "upper"
    inc = [f"-I{ref / 'include'}", f"-I{ref / 'external'}", f"-I{ref / 'external' / 'fmt' / 'include'}",
           f"-I{support}", f"-I{prec}", f"-I{upper / 'signal_processors'}", f"-I{upper / 'sequence_generators'}"]
    units = [upper / "signal_processors" / "dmrs_pdsch_processor_impl.cpp",
             upper / "sequence_generators" / "pseudo_random_generator_impl.cpp",
             support / "resource_grid_mapper_impl.cpp", support / "resource_grid_writer_impl.cpp",
             support / "re_pattern.cpp", prec / "channel_precoder_generic.cpp", prec / "channel_precoder_impl.cpp",
             lib / "srsvec" / "conversion.cpp", lib / "srsvec" / "sc_prod.cpp"]
    subprocess.run(["g++", *REF_FLAGS, *inc, "-shared", "-Wl,-z,defs", "-o", str(OUT), str(shim), *map(str, units)],
                   check=True)
    so = ctypes.CDLL(str(OUT))
    P, U = ctypes.c_void_p, ctypes.c_uint
    so.ref_dmrs.restype = ctypes.c_int
    so.ref_dmrs.argtypes = [U, U, U, U, U, P, U, U, U, U, ctypes.c_float, U, P, P, P, U, P]
    return so


def ref_case(so, c, w):
    """(cbf16 uint32 [P count], cf32 bits uint32 [P count 2]) as dmrs_ref.run_case gives them, from the reference"""
    w = np.ascontiguousarray(w, np.complex64)
    L, P, gp = c["layers"], c["ports"], c["grid_ports"]
    nsubc = c["nrb"] * R.NRE
    rb = R.case_rb_mask(c).astype(np.uint8)
    mask = R.case_mask(c)
    grid = np.full((gp, R.NSYMB, nsubc), R.GUARD, np.uint32)
    cap = np.zeros(2 * P * int(mask.sum()) + 16, np.float32)
    calls = ctypes.c_uint()
    n = so.ref_dmrs(gp, c["nrb"], c["type"], L, P, w.ctypes.data, c["slot"], c["ref"], c["id"], c["n_scid"],
                    c["amplitude"], sum(1 << l for l in c["symbols"]), rb.ctypes.data, grid.ctypes.data,
                    cap.ctypes.data, cap.size, ctypes.byref(calls))
    assert n == 2 * P * int(mask.sum()), "the reference mapped another number of REs"
    assert calls.value == (L + 1) // 2, "one mapper call per CDM group"
    assert np.all(grid[:P][:, ~mask] == R.GUARD) and np.all(grid[P:] == R.GUARD), "the reference wrote elsewhere"
    # the captured values of CDM group g: [port][symbol][RB][pilot j], onto the grid's (symbol, subcarrier)
    pre = np.full((P, R.NSYMB, nsubc, 2), R.GUARD, np.uint32)
    rbs = np.flatnonzero(rb)
    bits = cap[:n].view(np.uint32)
    at = 0
    for g in range((L + 1) // 2):
        k = (R.NRE * rbs[:, None] + R.pilot_subcarriers(c["type"], g)[None, :]).reshape(-1)
        per = k.size * len(c["symbols"])
        v = bits[at:at + 2 * P * per].reshape(P, len(c["symbols"]), k.size, 2)
        for i, l in enumerate(sorted(c["symbols"])):
            pre[:, l, k, :] = v[:, i]
        at += 2 * P * per
    assert at == n and np.all(pre[:, ~mask] == R.GUARD)
    return np.ascontiguousarray(grid[:P][:, mask]).reshape(-1), np.ascontiguousarray(pre[:, mask]).reshape(-1)


def main():
    # the reference tree: the argument, else oracle/Makefile's SRSRAN_REF
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_REF", "/root/reference"))
    so = build(ref)
    cases = R.cases()
    outs = []
    for c in cases:
        w = R.case_input(c)
        c["sha"] = digest(w)
        g, p = ref_case(so, c, w)
        # the recorded cf32 values round to the recorded grid
        f = p.view(np.float32).reshape(-1, 2)
        assert np.array_equal(R.P.to_cbf16(f[:, 0], f[:, 1]), g), c
        rg, rp = R.run_case(c, w)
        assert np.array_equal(g, rg) and np.array_equal(p, rp), f"the restatement differs from the reference: {c}"
        outs.append(np.concatenate([g, p]))
    off = np.cumsum([0] + [o.size for o in outs]).astype(np.int64)
    np.savez_compressed(R.GOLDEN, index=np.array(json.dumps(cases, separators=(",", ":"))), off=off,
                        out=np.concatenate(outs).astype(np.uint32))
    size = R.GOLDEN.stat().st_size
    print(f"{R.GOLDEN.name}: {len(cases)} cases, {sum(o.size // 3 for o in outs)} cbf16 REs with their cf32 values, "
          f"{size} bytes")
    for name, seen in R.fixture_classes(cases, [(o[:o.size // 3], o[o.size // 3:]) for o in outs]).items():
        assert seen, f"missing from the fixture: {name}"
    assert size <= MAX_BYTES, f"{R.GOLDEN.name}: {size} bytes"


if __name__ == "__main__":
    main()
