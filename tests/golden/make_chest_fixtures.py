"""Records tests/golden/ref_chest.npz from the reference's PUSCH DM-RS channel estimator.

    python tests/golden/make_chest_fixtures.py [REFERENCE_TREE]

Not run by any test. Compiles a small shim of our own (below: it only includes reference headers) together with the
reference tree's dmrs_pusch_estimator_impl.cpp, port_channel_estimator_average_impl.cpp, interpolator_linear_impl.cpp,
pseudo_random_generator_impl.cpp, resource_grid_reader_impl.cpp and the srsvec units they need, in place, with the flags
of oracle/Makefile's `ref` target (-O2 -march=x86-64 -ffp-contract=off: only the scalar loops are built), into the
git-ignored oracle/_ref/libsrsran_ref_chest.so. The shim provides two stand-ins: a time_alignment_estimator that returns
0 (the time alignment is outside this project's estimator, and its DFT stays out of the build), and an interpolator in
front of the reference's that records the filtered pilots it is handed and the cf32 values it gets back, and passes the
call on. The file holds, per case of tests/chest_ref.py's cases(), the parameters with the seed, the SHA-256 of the
received grid regenerated from the seed, and per (layer, rx port) plane the bit patterns of the filtered pilots, the
interpolated cf32 values, the cbf16 estimates of one symbol, epre, rsrp, noise variance, snr and cfo_Hz (NaN: none), and
the five raw sums of the float32 restatement behind them. The generator asserts that all symbols of the range are equal,
that everything else of the estimate keeps its guard, that the recorded cf32 values round to the recorded cbf16, and that
the restatement equals the reference in every bit.
tests/test_chest_host.py holds the NumPy restatement to it, tests/test_gpu_chest.py the HIP kernel."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import chest_ref as R  # noqa: E402
from tests.ref_cases import digest  # noqa: E402

MAX_BYTES = 106098  # as tests/golden/make_reference_fixtures.py allows
REF_FLAGS = "-std=c++17 -O2 -march=x86-64 -ffp-contract=off -fPIC -DASSERTS_ENABLED -DFMT_HEADER_ONLY -w".split()
OUT = ROOT / "oracle" / "_ref" / "libsrsran_ref_chest.so"

SHIM = r"""
#include "dmrs_pusch_estimator_impl.h"
#include "interpolator_linear_impl.h"
#include "port_channel_estimator_average_impl.h"
#include "pseudo_random_generator_impl.h"
#include "resource_grid_reader_impl.h"
#include "srsran/adt/tensor.h"
#include "srsran/phy/support/time_alignment_estimator/time_alignment_estimator.h"
#include "srsran/phy/upper/channel_estimation.h"
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>
using namespace srsran;
static_assert(sizeof(cbf16_t) == 4, "cbf16 is two bf16");

namespace {
class zero_ta : public time_alignment_estimator
{
public:
  time_alignment_measurement estimate(span<const cf_t>, bounded_bitset<max_nof_symbols>, subcarrier_spacing,
                                      double) override
  {
    return {0.0, 0.0, 0.0, 0.0};
  }
  time_alignment_measurement estimate(span<const cf_t>, unsigned, subcarrier_spacing, double) override
  {
    return {0.0, 0.0, 0.0, 0.0};
  }
};

std::vector<float> g_values; // per interpolate call: the input, then the output, as float pairs
unsigned           g_calls = 0;

class capture_interpolator : public interpolator
{
public:
  void interpolate(span<cf_t> output, span<const cf_t> input, const configuration& cfg) override
  {
    next.interpolate(output, input, cfg);
    ++g_calls;
    for (const cf_t& v : input) {
      g_values.push_back(v.real());
      g_values.push_back(v.imag());
    }
    for (const cf_t& v : output) {
      g_values.push_back(v.real());
      g_values.push_back(v.imag());
    }
  }
  interpolator_linear_impl next;
};
} // namespace

// grid: [port][symbol][subcarrier] cbf16; est: [layer][port][symbol < first + nsymb][subcarrier] cbf16, read (the
// guard) and written; metrics: [port][layer] epre, rsrp, noise variance, snr, cfo_Hz (NaN: none); captured: per
// (port, layer) in the reference's call order the 6 A filtered pilots and the 12 A interpolated values
extern "C" int ref_chest(unsigned grid_ports, unsigned nof_rb, unsigned L, unsigned P, const uint8_t* rx_ports,
                         unsigned numerology, unsigned slot_index, unsigned scrambling_id, unsigned n_scid,
                         float scaling, unsigned symbols, unsigned first, unsigned nsymb, const uint8_t* rb,
                         unsigned strategy, const uint32_t* grid, uint32_t* est, float* metrics, float* captured,
                         unsigned cap)
{
  const unsigned nof_subc = nof_rb * NRE;
  dynamic_tensor<3, cbf16_t, resource_grid_dimensions> data({nof_subc, MAX_NSYMB_PER_SLOT, grid_ports});
  std::memcpy(data.get_data().data(), grid, sizeof(cbf16_t) * data.get_data().size());
  std::atomic<unsigned>     empty{0};
  resource_grid_reader_impl reader(data, empty);

  dmrs_pusch_estimator::configuration config;
  config.slot          = slot_point(numerology, 0, slot_index);
  config.type          = dmrs_type::TYPE1;
  config.scrambling_id = scrambling_id;
  config.n_scid        = n_scid != 0;
  config.scaling       = scaling;
  config.c_prefix      = cyclic_prefix::NORMAL;
  config.symbols_mask  = bounded_bitset<MAX_NSYMB_PER_SLOT>(MAX_NSYMB_PER_SLOT);
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
  config.first_symbol  = first;
  config.nof_symbols   = nsymb;
  config.nof_tx_layers = L;
  for (unsigned p = 0; p != P; ++p) {
    config.rx_ports.push_back(rx_ports[p]);
  }

  channel_estimate::channel_estimate_dimensions dims;
  dims.nof_prb       = nof_rb;
  dims.nof_symbols   = first + nsymb;
  dims.nof_rx_ports  = P;
  dims.nof_tx_layers = L;
  channel_estimate ce(dims);
  const size_t     path = static_cast<size_t>(nof_subc) * (first + nsymb);
  for (unsigned l = 0; l != L; ++l) {
    for (unsigned p = 0; p != P; ++p) {
      span<cbf16_t> s = ce.get_path_ch_estimate(p, l);
      if (s.size() != path) {
        return -2;
      }
      std::memcpy(s.data(), est + (static_cast<size_t>(l) * P + p) * path, sizeof(cbf16_t) * path);
    }
  }

  g_values.clear();
  g_calls = 0;
  auto port_est = std::make_unique<port_channel_estimator_average_impl>(
      std::make_unique<capture_interpolator>(),
      std::make_unique<zero_ta>(),
      strategy == 1 ? port_channel_estimator_fd_smoothing_strategy::filter
                    : port_channel_estimator_fd_smoothing_strategy::none,
      false);
  dmrs_pusch_estimator_impl estimator(std::make_unique<pseudo_random_generator_impl>(), std::move(port_est));
  estimator.estimate(ce, reader, config);

  for (unsigned l = 0; l != L; ++l) {
    for (unsigned p = 0; p != P; ++p) {
      span<cbf16_t> s = ce.get_path_ch_estimate(p, l);
      std::memcpy(est + (static_cast<size_t>(l) * P + p) * path, s.data(), sizeof(cbf16_t) * path);
    }
  }
  for (unsigned p = 0; p != P; ++p) {
    for (unsigned l = 0; l != L; ++l) {
      float* m = metrics + 5 * (p * L + l);
      m[0]     = ce.get_epre(p, l);
      m[1]     = ce.get_rsrp(p, l);
      m[2]     = ce.get_noise_variance(p, l);
      m[3]     = ce.get_snr(p, l);
      m[4]     = ce.get_cfo_Hz(p, l).has_value() ? ce.get_cfo_Hz(p, l).value() : std::nanf("");
    }
  }
  if (g_calls != L * P || g_values.size() > cap) {
    return -1;
  }
  std::memcpy(captured, g_values.data(), sizeof(float) * g_values.size());
  return static_cast<int>(g_values.size());
}
"""


def build(ref: Path) -> ctypes.CDLL:
    lib = ref / "lib"
    OUT.parent.mkdir(parents=True, exist_ok=True)
    shim = OUT.parent / "ref_chest_shim.cpp"
    shim.write_text(SHIM)
    support, upper, vec = lib / "phy" / "support", lib / "phy" / "upper", lib / "srsvec"
    inc = [f"-I{ref / 'include'}", f"-I{ref / 'external'}", f"-I{ref / 'external' / 'fmt' / 'include'}",
           f"-I{support}", f"-I{support / 'interpolator'}", f"-I{upper / 'signal_processors'}",
           f"-I{upper / 'sequence_generators'}", f"-I{lib}"]
    units = [upper / "signal_processors" / "dmrs_pusch_estimator_impl.cpp",
             upper / "signal_processors" / "port_channel_estimator_average_impl.cpp",
             upper / "sequence_generators" / "pseudo_random_generator_impl.cpp",
             support / "interpolator" / "interpolator_linear_impl.cpp", support / "resource_grid_reader_impl.cpp",
             support / "re_pattern.cpp"]
    units += [vec / f"{n}.cpp" for n in ("add", "conversion", "convolution", "dot_prod", "prod", "sc_prod", "unwrap")]
    units = [u for u in units if u.exists()]
    subprocess.run(["g++", *REF_FLAGS, *inc, "-shared", "-Wl,-z,defs", "-o", str(OUT), str(shim), *map(str, units)],
                   check=True)
    so = ctypes.CDLL(str(OUT))
    P, U = ctypes.c_void_p, ctypes.c_uint
    so.ref_chest.restype = ctypes.c_int
    so.ref_chest.argtypes = [U, U, U, U, P, U, U, U, U, ctypes.c_float, U, U, U, P, U, P, P, P, P, U]
    return so


def ref_case(so, c, grid):
    """per plane (layer-major) the dict chest_ref.split_record gives, minus the sums, from the reference"""
    L, P = c["layers"], c["ports"]
    nsubc = c["nrb"] * R.NRE
    rb = R.case_rb_mask(c).astype(np.uint8)
    n = R.DPR * int(rb.sum())
    last = c["first"] + c["nsymb"]
    est = np.full((L, P, last, nsubc), R.GUARD, np.uint32)
    metrics = np.zeros((P, L, 5), np.float32)
    cap = np.zeros(L * P * 6 * n + 16, np.float32)
    rxp = np.array(c["rx_ports"], np.uint8)
    got = so.ref_chest(c["grid_ports"], c["nrb"], L, P, rxp.ctypes.data, c["numerology"], c["slot"], c["id"],
                       c["n_scid"], c["scaling"], sum(1 << l for l in c["symbols"]), c["first"], c["nsymb"],
                       rb.ctypes.data, c["strategy"], np.ascontiguousarray(grid).ctypes.data, est.ctypes.data,
                       metrics.ctypes.data, cap.ctypes.data, cap.size)
    assert got == L * P * 6 * n, f"the reference interpolated another number of values: {got}"
    k = (R.NRE * np.flatnonzero(rb)[:, None] + np.arange(R.NRE)[None, :]).reshape(-1)
    keep = np.ones(nsubc, bool)
    keep[k] = False
    assert np.all(est[:, :, :c["first"]] == R.GUARD) and np.all(est[:, :, :, keep] == R.GUARD), "guard overwritten"
    bits = cap[:got].view(np.uint32).reshape(P, L, 6 * n)
    out = []
    for layer in range(L):
        for p in range(P):
            rows = est[layer, p, c["first"]:last][:, k]
            assert np.all(rows == rows[0]), "the symbols of the range differ"
            out.append(dict(filtered=bits[p, layer, :2 * n].reshape(n, 2), interp=bits[p, layer, 2 * n:].reshape(2 * n, 2),
                            cbf16=rows[0].copy(), metrics=metrics[p, layer].view(np.uint32).copy()))
    return out


def main():
    # the reference tree: the argument, else oracle/Makefile's SRSRAN_REF
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_REF", "/root/reference"))
    so = build(ref)
    cases = R.cases()
    outs = []
    for c in cases:
        grid = R.case_input(c)
        c["sha"] = digest(grid)
        want = ref_case(so, c, grid)
        got = R.run_case(c, grid)
        words = []
        for i, (w, g) in enumerate(zip(want, got)):
            rec = R.plane_record(g)
            s = R.split_record(rec, w["filtered"].shape[0])
            f = w["interp"].view(np.float32)
            assert np.array_equal(R.P.to_cbf16(f[:, 0], f[:, 1]), w["cbf16"]), (c, i)
            for name in ("filtered", "interp", "cbf16"):
                assert np.array_equal(s[name], w[name]), f"the restatement's {name} differs from the reference: {c} {i}"
            a, b = s["metrics"].view(np.float32), w["metrics"].view(np.float32)
            assert np.array_equal(s["metrics"], w["metrics"]) or (np.isnan(a[4]) and np.isnan(b[4]) and
                                                                  np.array_equal(s["metrics"][:4], w["metrics"][:4])), \
                f"the restatement's metrics differ from the reference: {c} {i} {a} {b}"
            rec = rec.copy()
            rec[-10:-5] = w["metrics"]
            words.append(rec)
        outs.append(np.concatenate(words))
    off = np.cumsum([0] + [o.size for o in outs]).astype(np.int64)
    np.savez_compressed(R.GOLDEN, index=np.array(json.dumps(cases, separators=(",", ":"))), off=off,
                        out=np.concatenate(outs).astype(np.uint32))
    size = R.GOLDEN.stat().st_size
    print(f"{R.GOLDEN.name}: {len(cases)} cases, {sum(c['layers'] * c['ports'] for c in cases)} planes, {size} bytes")
    for name, seen in R.fixture_classes(cases).items():
        assert seen, f"missing from the fixture: {name}"
    assert size <= MAX_BYTES, f"{R.GOLDEN.name}: {size} bytes"


if __name__ == "__main__":
    main()
