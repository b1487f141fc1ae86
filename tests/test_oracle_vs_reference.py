"""CPU differential test: the oracle (oracle/ldpc_oracle.c and tests/scrambling_ref.py, the restatements every GPU test
compares a kernel with) against the reference itself, compiled by `make -C oracle ref` into
oracle/_ref/libsrsran_ref.so. Every comparison is exact equality of integers (tests/ref_cases.compare). The file
skips only where that library is absent (a checkout without the reference tree); the recorded fixtures
(tests/golden/ref_*.npz, tests/test_golden.py) still hold the oracle to the reference there.

Each test prints `<operation>: <compared> compared, <equal> equal`."""
import numpy as np
import pytest

import oracle as O
from oracle import ref
from tests import ref_cases as C

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref/libsrsran_ref.so is not built")


def _check(op, cases, inputs, run):
    n, eq, diffs = C.compare_cases(op, cases, inputs, run, C.ORACLE, ref)
    print(f"{op}: {n} compared, {eq} equal")
    assert n > 0 and not diffs, f"{op}: {len(diffs)} of {n} differ from the reference:\n" + "\n".join(diffs[:20])


def test_llr_arithmetic_exhaustive():
    """Saturating sum and promotion sum over every pair of legal LLRs; quantize on a grid with its rounding ties."""
    vals = list(range(-120, 121)) + [127, -127]
    bad = [(a, b) for a in vals for b in vals
           if O.llr_add(a, b) != ref.llr_add(a, b) or O.llr_promotion_sum(a, b) != ref.llr_promotion_sum(a, b)]
    print(f"llr pairs: {len(vals) ** 2} compared, {len(vals) ** 2 - len(bad)} equal")
    assert not bad, bad[:10]
    xs = np.concatenate([np.arange(-2000, 2001) / 240.0, np.arange(-2000, 2001) / 37.0]).astype(np.float32)
    badq = [(float(x), r) for r in (0.5, 8.0, 24.0) for x in xs if O.llr_quantize(x, r) != ref.llr_quantize(x, r)]
    assert not badq, badq[:10]


def test_decoder_all_graphs():
    cases = C.live_decode_cases()
    _check("decode", cases, [C.decode_input(c) for c in cases], C.run_decode)


def test_decoder_scaling_factors_cover_every_graph():
    """The case list itself: every (BG, Z) meets every scaling factor, 0.8 included, and iteration limits 1, 2, 10."""
    cases = C.live_decode_cases()
    seen = {(c["bg"], c["Z"], round(c["sf"], 6)) for c in cases}
    for bg, Z in C.GRAPHS:
        for sf in C.SFS_LIVE + [0.8]:
            assert (bg, Z, round(sf, 6)) in seen
    assert {1, 2, 10} <= {c["iters"] for c in cases}
    assert all(0 < c["sf"] < 1 for c in cases)


def test_decoder_early_stop_noisy():
    """Noisy codewords with CRC16 / CRC24A / CRC24B early stop and fillers on every graph whose K Z holds a CRC."""
    cases, inputs = C.noisy_decode_cases(C.GRAPHS, (1.0, 1.8, 2.1), 90000)
    _check("decode early stop", cases, inputs, C.run_decode)
    iters = [int(C.run_decode(ref, c, i)["iters"][0]) for c, i in zip(cases[::5], inputs[::5])]
    assert 0 in iters and len(set(iters)) >= 4, "the noise levels should give failures and several iteration counts"


def test_rate_dematcher():
    cases = C.live_dematch_cases()
    _check("rate dematch", cases, [C.dematch_input(c) for c in cases], C.run_dematch)


def test_dematch_decode_chains():
    cases = C.chain_cases()
    _check("dematch -> decode chain", cases, [C.chain_input(c) for c in cases], C.run_chain)


def test_demodulator_finite_inputs():
    cases = [c for c in C.demod_cases(2000) if c["group"] == "random"]
    _check("demodulate", cases, [C.demod_input(c) for c in cases], C.run_demod)


def test_demodulator_special_values_as_compiled():
    """NaN / infinite / out-of-range inputs: the reference converts them to int with undefined behaviour, so this
    group pins the reference as compiled by the committed recipe on x86-64, not the C++ standard."""
    cases = [c for c in C.demod_cases(2000) if c["group"] == "specials"]
    _check("demodulate specials", cases, [C.demod_input(c) for c in cases], C.run_demod)


def test_descrambler():
    cases = C.descramble_cases()
    _check("descramble", cases, [C.descramble_input(c) for c in cases], C.run_descramble)


def test_encoder_all_graphs():
    cases = C.encode_cases(shortened=True)
    _check("encode", cases, [C.encode_input(c) for c in cases], C.run_encode)


def test_rate_matcher():
    """rate_match_cases(), then the branch grid, every lifted graph and the staging rows of tests/rm_grid.py (all but
    the 'division' rows, whose E the reference does not take)."""
    cases = C.live_rate_match_cases()
    assert sum("row" in c for c in cases) == 342 + 66 - 4
    _check("rate match", cases, [C.rate_match_input(c) for c in cases], C.run_rate_match)


def test_encoder_on_the_rate_match_grid_messages():
    """The codewords the grid's rows are cut from: the oracle encoder against the reference's on every grid message."""
    from tests.rm_grid import all_rows
    rows = all_rows()
    cases = [dict(bg=c["bg"], Z=c["Z"], F=c["F"], L=O.BG_N_SHORT[c["bg"]] * c["Z"], seed=c["seed"]) for c in rows]
    _check("encode (rate match grid)", cases, [C.rm_message(c) for c in rows], C.run_encode)


def test_crc():
    cases = C.crc_cases()
    _check("crc", cases, [C.crc_input(c) for c in cases], C.run_crc)
