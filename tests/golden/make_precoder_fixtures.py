"""Records tests/golden/ref_precode.npz from the reference's resource grid mapper and channel precoder.

    python tests/golden/make_precoder_fixtures.py [REFERENCE_TREE]

Not run by any test. Compiles a small shim of our own (below: it only includes reference headers) together with the
reference tree's resource_grid_mapper_impl.cpp, resource_grid_writer_impl.cpp, re_pattern.cpp,
channel_precoder_generic.cpp, channel_precoder_impl.cpp, srsvec/conversion.cpp and srsvec/sc_prod.cpp, in place, with
the flags of oracle/Makefile's `ref` target (-O2 -march=x86-64 -ffp-contract=off: SRSRAN_SIMD_CF_SIZE is 0, so only the
scalar loops are built), into the git-ignored oracle/_ref/libsrsran_ref_precoder.so. The file holds, per case of
tests/precoder_ref.py's cases(), the parameters with the seed, the SHA-256 of the inputs regenerated from the seed, and
the bit patterns the reference wrote: for a grid case the masked REs of every port (the rest of the grid must still hold
the guard pattern), for a compact case the cf32 outputs of apply_layer_map_and_precoding and of apply_precoding.
tests/test_precoder_host.py holds the NumPy restatement to it, tests/test_gpu_precoder.py the HIP kernel."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from tests import precoder_ref as R  # noqa: E402
from tests.ref_cases import digest  # noqa: E402

MAX_BYTES = 106098  # as tests/golden/make_reference_fixtures.py allows
REF_FLAGS = "-std=c++17 -O2 -march=x86-64 -ffp-contract=off -fPIC -DASSERTS_ENABLED -DFMT_HEADER_ONLY -w".split()
OUT = ROOT / "oracle" / "_ref" / "libsrsran_ref_precoder.so"
MAX_RB = 275

SHIM = r"""
#include "channel_precoder_generic.h"
#include "resource_grid_mapper_impl.h"
#include "resource_grid_writer_impl.h"
#include "srsran/adt/tensor.h"
#include "srsran/phy/support/precoding_configuration.h"
#include "srsran/phy/support/re_pattern.h"
#include <atomic>
#include <cstring>
#include <memory>
using namespace srsran;
static_assert(sizeof(cbf16_t) == 4, "cbf16 is two bf16");
static_assert(sizeof(ci8_t) == 2, "ci8 is two int8");

static precoding_weight_matrix matrix(const float* w, unsigned L, unsigned P)
{
  precoding_weight_matrix m(L, P);
  for (unsigned p = 0; p != P; ++p) {
    for (unsigned l = 0; l != L; ++l) {
      m.set_coefficient(cf_t(w[2 * (p * L + l)], w[2 * (p * L + l) + 1]), l, p);
    }
  }
  return m;
}

// patterns: n entries of (MAX_RB PRB flags, 12-bit RE mask, 14-bit symbol mask)
static re_pattern_list patterns(unsigned n, const uint8_t* prb, const uint16_t* re, const uint16_t* sym)
{
  re_pattern_list list;
  for (unsigned i = 0; i != n; ++i) {
    re_pattern p;
    p.prb_mask = bounded_bitset<MAX_RB>(MAX_RB);
    for (unsigned b = 0; b != MAX_RB; ++b) {
      if (prb[i * MAX_RB + b]) {
        p.prb_mask.set(b);
      }
    }
    for (unsigned b = 0; b != NRE; ++b) {
      if ((re[i] >> b) & 1U) {
        p.re_mask.set(b);
      }
    }
    p.symbols = symbol_slot_mask(MAX_NSYMB_PER_SLOT);
    for (unsigned b = 0; b != MAX_NSYMB_PER_SLOT; ++b) {
      if ((sym[i] >> b) & 1U) {
        p.symbols.set(b);
      }
    }
    list.merge(p);
  }
  return list;
}

// grid: [port][symbol][subcarrier] cbf16, read and written; weights [prg][port][layer] with the scaling applied
extern "C" int ref_map(unsigned nof_ports, unsigned nof_subc, unsigned L, unsigned P, unsigned nof_prg,
                       unsigned prg_size, const float* weights, const int8_t* symbols, unsigned nof_symbols,
                       unsigned n_incl, const uint8_t* incl_prb, const uint16_t* incl_re, const uint16_t* incl_sym,
                       unsigned n_resv, const uint8_t* resv_prb, const uint16_t* resv_re, const uint16_t* resv_sym,
                       uint32_t* grid)
{
  dynamic_tensor<3, cbf16_t, resource_grid_dimensions> data({nof_subc, MAX_NSYMB_PER_SLOT, nof_ports});
  std::memcpy(data.get_data().data(), grid, sizeof(cbf16_t) * data.get_data().size());
  std::atomic<unsigned>     empty{~0U};
  resource_grid_writer_impl writer(data, empty);
  resource_grid_mapper_impl mapper(nof_ports, nof_subc, writer, std::make_unique<channel_precoder_generic>());
  precoding_configuration   config(L, P, nof_prg, prg_size);
  for (unsigned g = 0; g != nof_prg; ++g) {
    config.set_prg_coefficients(matrix(weights + 2 * g * P * L, L, P), g);
  }
  resource_grid_mapper::symbol_buffer_adapter buffer(
      span<const ci8_t>(reinterpret_cast<const ci8_t*>(symbols), nof_symbols));
  mapper.map(buffer, patterns(n_incl, incl_prb, incl_re, incl_sym), patterns(n_resv, resv_prb, resv_re, resv_sym),
             config, 0);
  std::memcpy(grid, data.get_data().data(), sizeof(cbf16_t) * data.get_data().size());
  return buffer.empty() ? 0 : 1;
}

// channel_precoder: output [port][re] cf32; input ci8 (layer-interleaved) or cf32 layer planes [layer][re]
extern "C" int ref_precode(unsigned nof_re, unsigned L, unsigned P, const float* weights, const int8_t* ci8_in,
                           const float* cf32_in, float* out_ci8, float* out_cf32)
{
  channel_precoder_generic      precoder;
  const precoding_weight_matrix m = matrix(weights, L, P);
  dynamic_re_buffer             in(L, nof_re), out(P, nof_re);
  in.resize(L, nof_re);
  out.resize(P, nof_re);
  precoder.apply_layer_map_and_precoding(out, span<const ci8_t>(reinterpret_cast<const ci8_t*>(ci8_in), nof_re * L), m);
  for (unsigned p = 0; p != P; ++p) {
    std::memcpy(out_ci8 + 2 * p * nof_re, out.get_slice(p).data(), sizeof(cf_t) * nof_re);
  }
  for (unsigned l = 0; l != L; ++l) {
    std::memcpy(in.get_slice(l).data(), cf32_in + 2 * l * nof_re, sizeof(cf_t) * nof_re);
  }
  precoder.apply_precoding(out, in, m);
  for (unsigned p = 0; p != P; ++p) {
    std::memcpy(out_cf32 + 2 * p * nof_re, out.get_slice(p).data(), sizeof(cf_t) * nof_re);
  }
  return 0;
}
"""


def build(ref: Path) -> ctypes.CDLL:
    lib = ref / "lib"
    OUT.parent.mkdir(parents=True, exist_ok=True)
    shim = OUT.parent / "ref_precoder_shim.cpp"
    shim.write_text(SHIM)
    support, prec = lib / "phy" / "support", lib / "phy" / "generic_functions" / "precoding"
    inc = [f"-I{ref / 'include'}", f"-I{ref / 'external'}", f"-I{ref / 'external' / 'fmt' / 'include'}",
           f"-I{support}", f"-I{prec}"]
    units = [support / "resource_grid_mapper_impl.cpp", support / "resource_grid_writer_impl.cpp",
             support / "re_pattern.cpp", prec / "channel_precoder_generic.cpp", prec / "channel_precoder_impl.cpp",
             lib / "srsvec" / "conversion.cpp", lib / "srsvec" / "sc_prod.cpp"]
    subprocess.run(["g++", *REF_FLAGS, *inc, "-shared", "-o", str(OUT), str(shim), *map(str, units)], check=True)
    so = ctypes.CDLL(str(OUT))
    P, U = ctypes.c_void_p, ctypes.c_uint
    so.ref_map.restype = so.ref_precode.restype = ctypes.c_int
    so.ref_map.argtypes = [U, U, U, U, U, U, P, P, U, U, P, P, P, U, P, P, P, P]
    so.ref_precode.argtypes = [U, U, U, P, P, P, P, P]
    return so


def _patterns(pats):
    n = len(pats)
    prb = np.zeros((max(n, 1), MAX_RB), np.uint8)
    re, sym = np.zeros(max(n, 1), np.uint16), np.zeros(max(n, 1), np.uint16)
    for i, (prbs, re_mask, symbols) in enumerate(pats):
        for b, e in prbs:
            prb[i, b:e] = 1
        re[i] = re_mask
        sym[i] = sum(1 << l for l in symbols)
    return n, prb, re, sym


def ref_grid(so, c, inp) -> np.ndarray:
    """uint32 [P count] as precoder_ref.run_grid gives it, from the reference"""
    sym, w = np.ascontiguousarray(inp[0], np.int8), np.ascontiguousarray(inp[1], np.complex64)
    masks = R.case_masks(c)
    nsubc = c["nrb"] * R.NRE
    grid = np.full((c["ports"], R.NSYMB, nsubc), R.GUARD, np.uint32)
    ni, iprb, ire, isym = _patterns(c["incl"])
    nr, rprb, rre, rsym = _patterns(c["resv"])
    left = so.ref_map(c["ports"], nsubc, c["layers"], c["ports"], w.shape[0], c["prg_size"], w.ctypes.data,
                      sym.ctypes.data, sym.shape[0], ni, iprb.ctypes.data, ire.ctypes.data, isym.ctypes.data, nr,
                      rprb.ctypes.data, rre.ctypes.data, rsym.ctypes.data, grid.ctypes.data)
    assert left == 0, "the reference left symbols in the buffer"
    assert np.all(grid[:, ~masks] == R.GUARD), "the reference wrote outside the masks"
    return np.ascontiguousarray(grid[:, masks]).reshape(-1)


def ref_compact(so, c, inp):
    ci8, x, w = (np.ascontiguousarray(a) for a in inp)
    P, n = c["ports"], c["n"]
    a, b = np.empty((P, n), np.complex64), np.empty((P, n), np.complex64)
    so.ref_precode(n, c["layers"], P, w.ctypes.data, ci8.ctypes.data, x.ctypes.data, a.ctypes.data, b.ctypes.data)
    return a.view(np.uint32).reshape(-1), b.view(np.uint32).reshape(-1)


def main():
    # the reference tree: the argument, else oracle/Makefile's SRSRAN_REF
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SRSRAN_REF", "/root/reference"))
    so = build(ref)
    cases = R.cases()
    outs, pre = [], []  # pre: the float32 bit patterns before any cbf16 conversion
    for c in cases:
        inp = R.case_input(c)
        c["sha"] = digest(*inp)
        if c["form"] == "grid":
            o = ref_grid(so, c, inp)
            # the values before the conversion are the restatement's, once its grid equals the reference's
            assert np.array_equal(o, R.run_grid(c, inp)), c
            re, im = R.map_values(R.case_masks(c), c["prg_size"], inp[1], inp[0])[2]
            pre.append(np.concatenate([R.bits_of(re).reshape(-1), R.bits_of(im).reshape(-1)]))
            outs.append(o)
        else:
            a, b = ref_compact(so, c, inp)
            pre += [a, b]
            outs.append(np.concatenate([a, b]))
    off = np.cumsum([0] + [o.size for o in outs]).astype(np.int64)
    np.savez_compressed(R.GOLDEN, index=np.array(json.dumps(cases, separators=(",", ":"))), off=off,
                        out=np.concatenate(outs).astype(np.uint32))
    size = R.GOLDEN.stat().st_size

    grid = [(c, o, R.case_masks(c)) for c, o in zip(cases, outs) if c["form"] == "grid"]
    compact = [c for c in cases if c["form"] == "compact"]
    allpre = np.concatenate(pre)
    need = float(((allpre & 0xFFFF) != 0).mean())
    print(f"{R.GOLDEN.name}: {len(grid)} grid cases ({sum(o.size for _, o, _ in grid)} cbf16 REs), {len(compact)} "
          f"compact cases ({sum(2 * c['n'] * c['ports'] for c in compact)} cf32 REs), {100 * need:.1f} % of "
          f"{allpre.size} components need rounding, {size} bytes")

    def words(m):  # the mask words a row has a bit in
        return {int(k) // 64 for k in np.flatnonzero(m)}

    def rows(m):
        return [r for r in m if r.any()]

    def comb(c, m, which):
        rr = rows(m)
        alloc = R.pattern_mask(c["incl"], c["nrb"])
        full = any(np.array_equal(r, a) for r, a in zip(m, alloc) if r.any())
        k = np.arange(m.shape[1]) % R.NRE
        return full and any(set(k[r]) == {i for i in range(R.NRE) if (which >> i) & 1} for r in rr)

    def partial_no_comb(m):
        for r in rows(m):
            nib = np.pad(r, (0, -r.size % 4)).reshape(-1, 4)
            cnt = nib.sum(axis=1)
            if ((cnt == 3).any()):
                return True
        return False

    def prg_class(c, m):
        if c["prg_size"] != 4:
            return False
        k = np.flatnonzero(m.any(axis=0))
        return len(set(k // 48)) >= 3 and k[0] % 48 != 0

    low, high = [o & 0xFFFF for _, o, _ in grid], [o >> 16 for _, o, _ in grid]
    classes = {
        "all ten topologies in the grid form": {(c["layers"], c["ports"]) for c, _, _ in grid} >= set(R.TOPOLOGIES),
        "all ten topologies in the compact form": {(c["layers"], c["ports"]) for c in compact} == set(R.TOPOLOGIES),
        "grids of 11, 25 and 52 RB": {c["nrb"] for c, _, _ in grid} == {11, 25, 52},
        "a row of ten mask words": any(len(words(r)) == 10 for _, _, m in grid for r in rows(m)),
        "an allocation that begins inside a mask word and ends inside another": any(
            np.flatnonzero(r)[0] % 64 != 0 and np.flatnonzero(r)[-1] % 64 != 63 and len(words(r)) >= 2
            for _, _, m in grid for r in rows(m)),
        "comb 0x555 on a DM-RS symbol beside full data symbols": any(comb(c, m, 0x555) for c, _, m in grid),
        "comb 0xAAA on a DM-RS symbol beside full data symbols": any(comb(c, m, 0xAAA) for c, _, m in grid),
        "a reserved single RE per RB (partial nibbles, no comb)": any(partial_no_comb(m) for _, _, m in grid),
        "a non-contiguous PRB allocation": any(
            np.any(np.diff(np.flatnonzero(r.reshape(-1, R.NRE).any(axis=1))) > 1) for _, _, m in grid for r in rows(m)),
        "prg_size 4 over three PRGs, not from a PRG boundary": any(prg_class(c, m) for c, _, m in grid),
        "one wideband PRG": any(c["prg_size"] == R.WIDEBAND for c, _, _ in grid),
        "an empty OFDM symbol between two that have REs": any(
            any(not m[l].any() and m[:l].any() and m[l + 1:].any() and R.pattern_mask(c["incl"], c["nrb"])[l].any()
                for l in range(R.NSYMB)) for c, _, m in grid),
        "a case of one masked RE": any(int(m.sum()) == 1 for _, _, m in grid),
        "a negative zero stored for L = 1 and a zero weight": any(
            c["weights"] == "zero" and c["layers"] == 1 and ((lo == 0x8000).any() or (hi == 0x8000).any())
            for (c, _, _), lo, hi in zip(grid, low, high)),
        "bf16 ties that round down and up": any(
            c["weights"] == "tie" and set(np.concatenate([lo, hi]) & 0x7FFF) == {0x3F80, 0x3F82}
            for (c, _, _), lo, hi in zip(grid, low, high)),
        "levels of all four QAM orders up to +-15": {c["qm"] for c in cases} == {2, 4, 6, 8} and all(
            int(np.abs(R.case_input(c)[0].astype(np.int32)).max()) == (1 << (c["qm"] // 2)) - 1
            for c in cases if c["form"] == "compact" or int(R.case_masks(c).sum()) > 16),
    }
    for name, seen in classes.items():
        assert seen, f"missing from the fixture: {name}"
    assert need >= 0.90, "fewer than 90 % of the recorded components need rounding"
    assert size <= MAX_BYTES, f"{R.GOLDEN.name}: {size} bytes"


if __name__ == "__main__":
    main()
