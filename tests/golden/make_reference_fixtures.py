"""Records tests/golden/ref_*.npz, ref_dematch_grid.json and ref_rate_match_grid.json (digests only) from the compiled
reference (oracle/_ref/libsrsran_ref.so, `make -C oracle ref`).

    python tests/golden/make_reference_fixtures.py

Not run by any test. Each file holds, per case, the case's parameters with its seed and the SHA-256 of the input that
tests/ref_cases.py regenerates from the seed, and what the reference wrote for that input. Only the noisy codewords
of the early-stop set are stored as they are (they depend on a float normal draw). tests/test_golden.py holds the
oracle to these files everywhere and the live reference to them where it is built;
tests/test_gpu_reference_fixtures.py holds the HIP kernels to them."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

import oracle as O  # noqa: E402
from oracle import ref  # noqa: E402
from tests import ref_cases as C  # noqa: E402

MAX_BYTES = 106098  # the largest fixture that was here before these (c2.npz)
EARLY_STOP_GRAPHS = [(1, 11), (1, 52), (1, 160), (2, 36), (2, 144), (2, 208)]
EARLY_STOP_NOISES = (1.0, 1.7, 2.0, 2.4)


def early_stop_len(bg, Z):
    """Full length up to Z = 52; the larger graphs at (K + 12) Z + 5 LLRs, so that the stored inputs stay small."""
    return None if Z <= 52 else (O.BG_K[bg] + 12) * Z + 5


def record(op, cases, inputs, stored=False):
    run = C.OPS[op][1]
    outs = []
    for c, inp in zip(cases, inputs):
        c["sha"] = C.input_digest(inp)
        outs.append(run(ref, c, inp))
    path = C.GOLDEN / f"ref_{op}.npz"
    np.savez_compressed(path, **C.pack_fixture(cases, outs, inputs if stored else None))
    size = path.stat().st_size
    assert size <= MAX_BYTES, f"{path.name}: {size} bytes"
    print(f"{path.name}: {len(cases)} cases, {size} bytes")
    return outs


def record_dematch_grid():
    """tests/golden/ref_dematch_grid.json: per case of tests/dematch_grid.py its numbers and one SHA-256 over the three
    soft buffers the reference wrote (no buffer is stored: the full-size graphs' would not fit)."""
    import json
    from tests.dematch_grid import grid_cases
    cases = grid_cases()
    doc = {"keys": list(C.DEMATCH_GRID_KEYS), "cases": [[c[k] for k in C.DEMATCH_GRID_KEYS] for c in cases],
           "sha256": [C.dematch_grid_digest(ref, c) for c in cases]}
    path = C.GOLDEN / "ref_dematch_grid.json"
    path.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    assert path.stat().st_size <= MAX_BYTES, f"{path.name}: {path.stat().st_size} bytes"
    print(f"{path.name}: {len(cases)} cases, {path.stat().st_size} bytes")


def record_rate_match_grid():
    """tests/golden/ref_rate_match_grid.json: per row of tests/rm_grid.py the reference takes (all but the 'division'
    rows) its numbers and the SHA-256 of the packed output the reference wrote for the oracle encoder's codeword."""
    import json
    from tests.rm_grid import reference_rows
    cases = reference_rows()
    doc = {"keys": list(C.RM_GRID_KEYS), "cases": [[c[k] for k in C.RM_GRID_KEYS] for c in cases],
           "sha256": [C.rm_grid_digest(ref, c) for c in cases]}
    path = C.GOLDEN / "ref_rate_match_grid.json"
    path.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    assert path.stat().st_size <= MAX_BYTES, f"{path.name}: {path.stat().st_size} bytes"
    print(f"{path.name}: {len(cases)} cases, {path.stat().st_size} bytes")


def main():
    assert ref.available(), "build oracle/_ref first: make -C oracle ref"
    record_dematch_grid()
    record_rate_match_grid()
    for op, cases in (("decode", C.fixture_decode_cases()), ("decode_sf", C.fixture_decode_sf_cases()),
                      ("dematch", C.fixture_dematch_cases()), ("chain", C.chain_cases()),
                      ("demod", C.demod_cases(257)), ("descramble", C.descramble_cases()),
                      ("encode", C.encode_cases()), ("rate_match", C.rate_match_cases(full=False))):
        record(op, cases, [C.OPS[op][0](c) for c in cases])
    cases, inputs = C.noisy_decode_cases(EARLY_STOP_GRAPHS, EARLY_STOP_NOISES, 5000, cb_len=early_stop_len)
    outs = record("early_stop", cases, inputs, stored=True)
    # from the reference's outputs alone: the set can tell an early stop, a failure and the iteration count apart
    iters = [int(o["iters"][0]) for o in outs]
    print("early stop iterations:", iters)
    assert any(0 < i < 10 for i in iters), "no CB stops before the last iteration"
    assert 0 in iters, "no CB fails"
    assert len({i for i in iters if i}) >= 2, "fewer than two distinct iteration counts"
    assert {c["crc"] for c in cases} == set(C.CRCS) and any(c["F"] for c in cases)


if __name__ == "__main__":
    main()
