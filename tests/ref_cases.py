"""Cases and the one comparison function shared by the live differential test (tests/test_oracle_vs_reference.py:
oracle against the compiled reference), the fixture generator (tests/golden/make_reference_fixtures.py) and the fixture
checks (tests/test_golden.py, tests/test_gpu_reference_fixtures.py).

A case is a dict of plain numbers (it goes into a fixture's JSON index as it is). `<op>_input(case)` regenerates the
case's input from its seed with tests/vectors.py's splitmix64 generators; `run_<op>(impl, case, inp)` runs one
implementation and returns {name: integer array}. An implementation is a namespace with the oracle's call shapes:
ORACLE (the restatements in oracle/ and tests/scrambling_ref.py) or oracle.ref (the compiled reference).

All inputs stay inside what the reference asserts: LLRs in [-120, 120] or +-127, legal lengths, 0 < sf < 1."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import oracle as O
from tests import scrambling_ref as R
from tests.vectors import codeword_llrs, sm_bits, sm_ints, sm_llrs, sm_symbols

ORACLE = SimpleNamespace(ldpc_decode=O.ldpc_decode, rate_dematch=O.rate_dematch, rate_match=O.rate_match,
                         ldpc_encode=O.ldpc_encode, demodulate_soft=O.demodulate_soft, descramble=R.descramble,
                         xor_packed=R.xor_packed, crc_bits=O.crc_bits, crc_packed=O.crc_packed)

GRAPHS = [(bg, Z) for bg in (1, 2) for Z in O.LIFTING_SIZES]
SFS_FIXTURE = [0.5, 0.75, 0.9, 1 / 3]
SFS_LIVE = SFS_FIXTURE + [0.05, 0.99]
CRCS = [O.CRC16, O.CRC24A, O.CRC24B]
DM_STAGE = 32768
MODS = [0, 1, 2, 4, 6, 8]


def digest(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + b":" + a.tobytes())
    return h.hexdigest()


# ---- the comparison function --------------------------------------------------------------------------------------
def compare(got: dict, want: dict) -> list:
    """Names whose integer arrays differ (exact equality; a missing name or another shape differs)."""
    bad = []
    for k in want:
        a, b = np.asarray(got.get(k, [])), np.asarray(want[k])
        if a.shape != b.shape or not np.array_equal(a.astype(np.int64), b.astype(np.int64)):
            bad.append(k)
    return bad


def compare_cases(op: str, cases, inputs, run, a, b):
    """Runs implementations a and b over the cases; returns (compared, equal, [descriptions of the differing ones])."""
    diffs = []
    for c, inp in zip(cases, inputs):
        bad = compare(run(a, c, inp), run(b, c, inp))
        if bad:
            diffs.append(f"{op} {json.dumps({k: v for k, v in c.items() if k != 'sha'})}: {bad}")
    return len(cases), len(cases) - len(diffs), diffs


# ---- decoder --------------------------------------------------------------------------------------------------------
def has_crc_room(bg, Z, F=0):
    return O.BG_K[bg] * Z - F >= 32


def filler_of(Z):
    return Z // 2 + 8


def decode_case(bg, Z, L, kind, seed, iters, crc=O.NO_CRC, F=0, sf=0.8, **extra):
    return dict(bg=bg, Z=Z, L=L, kind=kind, seed=seed, iters=iters, crc=crc, F=F, sf=sf, **extra)


def decode_input(c):
    """kinds: 'mixed'; 'tailzero' (the last c['tz'] LLRs zero: fewer layers run); 'zero'; 'almost' (one non-zero LLR at
    c['nz']); filler positions (F > 0) hold +127 as the rate dematcher leaves them. 'noisy' inputs are not regenerated:
    they come with the case (noisy_decode_cases) or from the fixture."""
    bg, Z, L = c["bg"], c["Z"], c["L"]
    if c["kind"] in ("zero", "almost"):
        v = np.zeros(L, np.int8)
        if c["kind"] == "almost":
            v[c["nz"]] = c["val"]
        return v
    v = sm_llrs(c["seed"], L, "mixed")
    if c["kind"] == "tailzero":
        v[L - c["tz"]:] = 0
    if c["F"]:
        k = (O.BG_K[bg] - 2) * Z
        v[k - c["F"]:k] = 127
    return v


def run_decode(impl, c, llr):
    out, it = impl.ldpc_decode(c["bg"], c["Z"], llr, c["iters"], c["crc"], c["F"], c["sf"])
    return {"msg": out, "ok": np.array([it is not None], np.uint8), "iters": np.array([it or 0], np.uint8)}


def lengths(bg, Z):
    K, N = O.BG_K[bg], O.BG_N_SHORT[bg]
    return N * Z, (K + 2) * Z + 1, N * Z - 3


def fixture_decode_cases():
    """Every graph: one full-length and one shortened mixed CB, 3 iterations, default scaling factor."""
    cases = []
    for g, (bg, Z) in enumerate(GRAPHS):
        full, short, _ = lengths(bg, Z)
        cases.append(decode_case(bg, Z, full, "mixed", 1000 + g, 3))
        cases.append(decode_case(bg, Z, short if g % 2 else lengths(bg, Z)[2], "mixed", 2000 + g, 3))
    return cases


def fixture_decode_sf_cases():
    """Every graph: one CB at each non-default scaling factor, 3 iterations; lengths alternate full / shortened."""
    cases = []
    for g, (bg, Z) in enumerate(GRAPHS):
        for k, sf in enumerate(SFS_FIXTURE):
            L = lengths(bg, Z)[(g + k) % 3]
            cases.append(decode_case(bg, Z, L, "mixed", 3000 + 10 * g + k, 3, sf=sf))
    return cases


def live_decode_cases():
    """The differential test's decoder cases that need no encoder (see noisy_decode_cases for the others)."""
    cases = []
    for g, (bg, Z) in enumerate(GRAPHS):
        full, short, odd = lengths(bg, Z)
        cases.append(decode_case(bg, Z, full, "mixed", 11000 + g, 2))
        cases.append(decode_case(bg, Z, short, "mixed", 12000 + g, 10))
        cases.append(decode_case(bg, Z, odd, "mixed", 13000 + g, 1))
        cases.append(decode_case(bg, Z, full, "tailzero", 14000 + g, 2, tz=(5 + g % 7) * Z + 2))
        if has_crc_room(bg, Z, filler_of(Z)):
            cases.append(decode_case(bg, Z, full, "mixed", 15000 + g, 2, crc=CRCS[g % 3], F=filler_of(Z)))
        for k, sf in enumerate(SFS_LIVE):
            cases.append(decode_case(bg, Z, lengths(bg, Z)[(g + k) % 3], "mixed", 16000 + 10 * g + k, (1, 2, 10)[k % 3]
                                     if Z <= 96 else 2, sf=sf))
    # the all-zero and almost-zero rules, with and without a CRC (ldpc_decoder_impl.cpp:85-94)
    for bg, Z in [(1, 2), (2, 7), (1, 52), (2, 208), (1, 384)]:
        full, short, _ = lengths(bg, Z)
        for crc in (O.NO_CRC, O.CRC24B if has_crc_room(bg, Z) else O.NO_CRC):
            cases.append(decode_case(bg, Z, full, "zero", 0, 2, crc=crc))
            cases.append(decode_case(bg, Z, short, "zero", 0, 2, crc=crc))
            for nz, val in ((0, 5), (0, -127), (short - 1, 1), (full - 1, -120), (2 * Z, 127)):
                cases.append(decode_case(bg, Z, full, "almost", 0, 2, crc=crc, nz=nz, val=val))
    return cases


def noisy_decode_cases(graphs, noises, seed0, with_filler=True, cb_len=None):
    """Noisy codewords (random message + CRC -> encoder -> +-2 + N(0, noise) -> quantize) with early stop, 10
    iterations: per graph one CB per noise level, the CRC polynomial and the filler count rotating. The LLRs depend
    on a float normal draw, so they travel with the case: returns (cases, inputs)."""
    cases, inputs = [], []
    for g, (bg, Z) in enumerate(graphs):
        for k, noise in enumerate(noises):
            crc = CRCS[(g + k) % 3]
            F = filler_of(Z) if with_filler and (g + k) % 2 == 1 else 0
            if not has_crc_room(bg, Z, F):
                continue
            L = cb_len(bg, Z) if cb_len else None
            rng = np.random.default_rng(seed0 + 100 * g + k)
            llr, _ = codeword_llrs(rng, bg, Z, 2.0, noise, F=F, crc=crc, cb_len=L)
            cases.append(decode_case(bg, Z, llr.size, "noisy", seed0 + 100 * g + k, 10, crc=crc, F=F, noise=noise))
            inputs.append(llr)
    return cases, inputs


# ---- rate dematcher -------------------------------------------------------------------------------------------------
def dematch_case(bg, Z, E, rv, Qm, F, Nref, seed):
    return dict(bg=bg, Z=Z, E=E, rv=rv, Qm=Qm, F=F, Nref=Nref, seed=seed)


def dematch_input(c):
    """(start buffer, first transmission, retransmission): 'harq' LLRs, so +-127 of both signs, +-120 and small values
    meet each other in the combine."""
    N = O.BG_N_SHORT[c["bg"]] * c["Z"]
    return (sm_llrs(c["seed"], N, "harq"), sm_llrs(c["seed"] + 1, c["E"], "harq"),
            sm_llrs(c["seed"] + 2, c["E"], "harq"))


def run_dematch(impl, c, inp):
    """soft_new: the start buffer after a new-data pass; soft_comb: that buffer after a combining pass of the second
    transmission; soft_comb0: the start buffer itself combined with the first transmission (new_data false)."""
    start, tx1, tx2 = inp
    a = start.copy()
    impl.rate_dematch(a, tx1, True, c["rv"], c["Qm"], c["Nref"], c["F"])
    soft_new = a.copy()
    impl.rate_dematch(a, tx2, False, c["rv"], c["Qm"], c["Nref"], c["F"])
    b = start.copy()
    impl.rate_dematch(b, tx1, False, c["rv"], c["Qm"], c["Nref"], c["F"])
    return {"soft_new": soft_new, "soft_comb": a, "soft_comb0": b}


_HAL_DM_CASES = [  # tests/test_gpu_hal.py DM_CASES: (bg, Z, E, rv, Qm, F, Nref)
    (1, 384, 9728, 0, 8, 0, 0), (1, 384, 9760, 2, 8, 0, 0), (2, 36, 1248, 0, 2, 88, 0), (2, 36, 1248, 3, 2, 88, 0),
    (2, 52, 3000, 2, 4, 20, 0), (1, 52, 1500, 3, 6, 0, 2000), (2, 208, 4000, 1, 1, 100, 0),
    (1, 20, 3000, 0, 2, 0, 0), (2, 8, 1400, 1, 2, 8, 0), (1, 384, 60000, 0, 4, 0, 0), (2, 104, 300, 3, 6, 0, 3000),
    (1, 120, 4000, 1, 8, 64, 5000), (2, 384, 20000, 2, 4, 400, 0),
]
_EDGE_DM_CASES = [  # E around DM_STAGE (the LDS staging limit), E % 16 != 0, E / Qm < 64
    (2, 8, DM_STAGE - 1, 0, 1, 0, 0), (2, 8, DM_STAGE + 1, 1, 1, 8, 0), (2, 8, DM_STAGE - 2, 2, 2, 0, 0),
    (2, 8, DM_STAGE + 2, 3, 2, 8, 300), (1, 12, DM_STAGE - 8, 0, 8, 12, 0), (1, 12, DM_STAGE + 8, 2, 8, 0, 700),
    (2, 16, DM_STAGE, 1, 4, 0, 0), (2, 16, 1002, 0, 6, 28, 0), (1, 12, 777, 3, 1, 0, 0), (2, 36, 63 * 8, 0, 8, 88, 0),
    (1, 20, 10 * 6, 2, 6, 0, 0), (2, 8, 2, 0, 2, 0, 0), (2, 52, 31 * 4, 1, 4, 20, 0),
]


def live_dematch_cases():
    from tests.test_rm_reference_table import GRAPHS as RM_GRAPHS, REF_TABLE
    cases = [dematch_case(*t, 21000 + 3 * i) for i, t in enumerate(_HAL_DM_CASES + _EDGE_DM_CASES)]
    for i, (E, rv, Qm, nref, lbrm, F) in enumerate(REF_TABLE):
        for j, (bg, Z) in enumerate(RM_GRAPHS):
            cases.append(dematch_case(bg, Z, E, rv, Qm, F, nref if lbrm else 0, 22000 + 10 * i + 3 * j))
    # every branch of the allot loop on graphs of every decoder body, and E / Qm around every workgroup width
    # (tests/dematch_grid.py). The reference accepts every row, the empty transmission included.
    from tests.dematch_grid import grid_cases
    return cases + grid_cases()


def dematch_grid_digest(impl, c) -> str:
    """One SHA-256 over a grid case's three results (tests/golden/ref_dematch_grid.json records the reference's)."""
    r = run_dematch(impl, c, dematch_input(c))
    return digest(r["soft_new"], r["soft_comb"], r["soft_comb0"])


DEMATCH_GRID_KEYS = ("bg", "Z", "E", "rv", "Qm", "F", "Nref", "seed", "row", "kind")


def load_dematch_grid():
    """[(case, recorded digest)] of tests/golden/ref_dematch_grid.json: case numbers and digests only."""
    d = json.loads((Path(__file__).resolve().parent / "golden" / "ref_dematch_grid.json").read_text())
    assert d["keys"] == list(DEMATCH_GRID_KEYS)
    return [(dict(zip(d["keys"], row)), sha) for row, sha in zip(d["cases"], d["sha256"])]


def fixture_dematch_cases():
    """16 of the live cases whose soft buffers are small enough to store, one full-size one included."""
    small = [t for t in _HAL_DM_CASES if O.BG_N_SHORT[t[0]] * t[1] <= 3500][:6] + [_HAL_DM_CASES[0]]
    edge = _EDGE_DM_CASES[:9]
    return [dematch_case(*t, 23000 + 3 * i) for i, t in enumerate(small + edge)]


# ---- dematch -> decode chains (rv 0, then rv 2 combined into the same soft buffer) ---------------------------------
def chain_cases():
    out = []
    for i, (bg, Z, Qm, E, F, crc) in enumerate([(2, 36, 2, 1248, 88, O.CRC16), (1, 12, 4, 600, 0, O.CRC24B),
                                                (2, 52, 6, 1500, 34, O.CRC24A), (1, 20, 8, 1200, 18, O.CRC24B),
                                                (2, 16, 1, 501, 0, O.CRC16), (1, 52, 2, 3000, 0, O.CRC24A)]):
        out.append(dict(bg=bg, Z=Z, Qm=Qm, E=E, F=F, crc=crc, iters=4, seed=31000 + 5 * i))
    return out


def chain_input(c):
    return sm_llrs(c["seed"], c["E"], "harq"), sm_llrs(c["seed"] + 1, c["E"], "mixed")


def run_chain(impl, c, inp):
    N = O.BG_N_SHORT[c["bg"]] * c["Z"]
    soft = np.zeros(N, np.int8)
    res = {}
    for k, (rv, tx) in enumerate(zip((0, 2), inp)):
        impl.rate_dematch(soft, tx, k == 0, rv, c["Qm"], 0, c["F"])
        res[f"soft{k}"] = soft.copy()
        msg, it = impl.ldpc_decode(c["bg"], c["Z"], soft, c["iters"], c["crc"], c["F"])
        res[f"msg{k}"] = msg
        res[f"iters{k}"] = np.array([it or 0], np.uint8)
    return res


# ---- demodulator ------------------------------------------------------------------------------------------------------
def demod_cases(n=257):
    cases = [dict(mod=mod, n=n, seed=41000 + mod, group=grp) for mod in MODS for grp in ("random", "specials")]
    # the input that showed the oracle and the kernel quantising 16-QAM over +-24 where the reference uses +-20
    next(c for c in cases if c["mod"] == 4 and c["group"] == "random")["name"] = "qam16_range_limit_20"
    return cases


def demod_input(c):
    """'random': noisy constellation points with per-symbol noise variances. 'specials': the special values of
    tests/test_gpu_demod.py::test_demod_special_values on top of them. A float-to-int conversion of NaN or of an
    out-of-range value is undefined C++ in the reference, so that group pins the reference as compiled by the
    committed recipe on x86-64."""
    sym, nv = sm_symbols(c["seed"], c["n"], c["mod"], 0.02 if c["group"] == "specials" else 0.1)
    if c["group"] == "specials":
        inf = np.float32(np.inf)
        nv[0::11] = 0.0
        nv[1::13] = np.inf
        nv[2::17] = -2.0
        nv[3::19] = np.nan
        nv[4::23] = 1e-30
        sym[5::12] = 0
        sym[6::29] = complex(inf, 0)
        sym[7::31] = complex(-inf, inf)
        sym[8::37] = complex(0, -inf)
        sym[9::41] = complex(np.nan, 0)
        sym[10::43] = 1e-6 + 1e-6j
        sym[11::47] = 1e6 - 1e6j
    return sym, nv


def run_demod(impl, c, inp):
    return {"llr": impl.demodulate_soft(c["mod"], *inp)}


# ---- descrambler ------------------------------------------------------------------------------------------------------
def descramble_cases():
    rows = [(0x2468ACE, 0, 1), (0x2468ACE, 0, 32), (1, 7, 33), (0x7FFFFFFF, 0, 1247), (0x091A0155, 1248, 1248),
            (0x5A5A5A5, 31, 4096), (12345, 70000, 515), (0x40000001, 3, 9728)]
    return [dict(c_init=ci, offset=off, n=n, seed=51000 + i) for i, (ci, off, n) in enumerate(rows)]


def descramble_input(c):
    return sm_llrs(c["seed"], c["n"], "mixed")


def run_descramble(impl, c, llr):
    bits = (llr.astype(np.int16) & 1).astype(np.uint8)
    return {"llr": impl.descramble(llr, c["c_init"], c["offset"]),
            "packed": impl.xor_packed(np.packbits(bits), c["c_init"], c["offset"], c["n"])}


# ---- encoder and rate matcher -------------------------------------------------------------------------------------------
def encode_cases(shortened=False):
    cases = []
    for g, (bg, Z) in enumerate(GRAPHS):
        full, short, odd = lengths(bg, Z)
        F = min(filler_of(Z), (O.BG_K[bg] - 2) * Z - 1)
        cases.append(dict(bg=bg, Z=Z, F=F, L=full, seed=61000 + g))
        if shortened:
            cases.append(dict(bg=bg, Z=Z, F=0, L=(short, odd)[g % 2], seed=62000 + g))
    return cases


def encode_input(c):
    KZ = O.BG_K[c["bg"]] * c["Z"]
    msg = sm_bits(c["seed"], KZ)
    if c["F"]:
        msg[KZ - c["F"]:] = O.FILLER_BIT
    return msg


def run_encode(impl, c, msg):
    cw = impl.ldpc_encode(c["bg"], c["Z"], msg, c["L"])
    return {"fill": np.flatnonzero(cw == O.FILLER_BIT)[[0, -1]] if c["F"] else np.zeros(2, np.int64),
            "cw": np.packbits(np.where(cw == O.FILLER_BIT, 0, cw).astype(np.uint8))}


def rate_match_cases(full=True):
    """All RVs, Qm in {1, 2, 4, 6, 8}, Nref limited and not, with and without fillers."""
    graphs = [(2, 16), (1, 12), (2, 52), (1, 36)]
    cases = []
    i = 0
    for rv in range(4):
        for Qm in (1, 2, 4, 6, 8):
            for lim in ((0, 1) if full else (((rv + Qm) // 2) % 2,)):
                bg, Z = graphs[i % 4]
                N = O.BG_N_SHORT[bg] * Z
                E = Qm * ((N * (3 + i % 5) // 4 + 13 * i) // Qm)
                cases.append(dict(bg=bg, Z=Z, E=E, rv=rv, Qm=Qm, Nref=(N * 2 // 3 + 1) if lim else 0,
                                  F=(0, filler_of(Z))[i % 2], seed=71000 + i))
                i += 1
    return cases


def rm_message(c):
    """A grid case's message (tests/rm_grid.py): K Z seeded bits, the oracle's FILLER_BIT at the last F positions."""
    KZ = O.BG_K[c["bg"]] * c["Z"]
    msg = sm_bits(c["seed"], KZ)
    if c["F"]:
        msg[KZ - c["F"]:] = O.FILLER_BIT
    return msg


def rate_match_input(c):
    """A codeblock's worth of random bits with the filler positions marked (the rate matcher does not look at whether
    they form a codeword, so no encoder is involved). A case of tests/rm_grid.py (it names its row) gets the oracle
    encoder's codeword of rm_message instead: the fused encoder route can be given nothing else."""
    if "row" in c:
        return O.ldpc_encode(c["bg"], c["Z"], rm_message(c))
    N = O.BG_N_SHORT[c["bg"]] * c["Z"]
    cw = sm_bits(c["seed"], N)
    k = (O.BG_K[c["bg"]] - 2) * c["Z"]
    cw[k - c["F"]:k] = O.FILLER_BIT
    return cw


def run_rate_match(impl, c, cw):
    return {"bits": np.packbits(impl.rate_match(cw, c["E"], c["rv"], c["Qm"], c["Nref"], c["bg"], c["Z"]))}


def live_rate_match_cases():
    """The differential test's rate matcher cases: rate_match_cases(), then every row of tests/rm_grid.py the reference
    takes (the branch grid, every lifted graph, the staging rows without the 'division' ones)."""
    from tests.rm_grid import reference_rows
    return rate_match_cases() + reference_rows()


def rm_grid_digest(impl, c, cw=None) -> str:
    """SHA-256 of a grid case's packed output (tests/golden/ref_rate_match_grid.json records the reference's)."""
    return digest(run_rate_match(impl, c, rate_match_input(c) if cw is None else cw)["bits"])


RM_GRID_KEYS = ("bg", "Z", "E", "rv", "Qm", "Nref", "F", "seed", "row", "kind")


def load_rm_grid():
    """[(case, recorded digest)] of tests/golden/ref_rate_match_grid.json: case numbers and digests only."""
    d = json.loads((Path(__file__).resolve().parent / "golden" / "ref_rate_match_grid.json").read_text())
    assert d["keys"] == list(RM_GRID_KEYS)
    return [(dict(zip(d["keys"], row)), sha) for row, sha in zip(d["cases"], d["sha256"])]


# ---- CRC --------------------------------------------------------------------------------------------------------------
def crc_cases():
    return [dict(poly=p, n=int(n), seed=81000 + 7 * i + p)
            for p in CRCS for i, n in enumerate(sm_ints(80000 + p, 12, 1, 9000))]


def crc_input(c):
    return sm_bits(c["seed"], c["n"])


def run_crc(impl, c, bits):
    return {"crc": np.array([impl.crc_bits(c["poly"], bits), impl.crc_packed(c["poly"], np.packbits(bits), c["n"])])}


# ---- fixture files: one .npz per operation -----------------------------------------------------------------------
def pack_fixture(cases, outputs, stored_inputs=None) -> dict:
    """{'index': JSON of the cases, '<name>': every case's array of that name concatenated, '<name>_off': offsets}."""
    d = {"index": np.array(json.dumps(cases))}
    for name in outputs[0]:
        arrs = [np.asarray(o[name]).ravel() for o in outputs]
        d[name] = np.concatenate(arrs)
        d[name + "_off"] = np.cumsum([0] + [a.size for a in arrs]).astype(np.int64)
    if stored_inputs is not None:
        d["in"] = np.concatenate(stored_inputs)
        d["in_off"] = np.cumsum([0] + [a.size for a in stored_inputs]).astype(np.int64)
    return d


def unpack_fixture(d):
    """(cases, [outputs dict per case], [stored input per case] or None)."""
    cases = json.loads(str(d["index"]))
    names = [k for k in d.files if k != "index" and not k.endswith("_off") and k != "in"]
    outs = [{k: d[k][d[k + "_off"][i]:d[k + "_off"][i + 1]] for k in names} for i in range(len(cases))]
    ins = [d["in"][d["in_off"][i]:d["in_off"][i + 1]] for i in range(len(cases))] if "in" in d.files else None
    return cases, outs, ins


# operation -> (input function, run function); the fixture generator and the fixture checks walk this table
OPS = {
    "decode": (decode_input, run_decode), "decode_sf": (decode_input, run_decode),
    "early_stop": (None, run_decode), "dematch": (dematch_input, run_dematch), "chain": (chain_input, run_chain),
    "demod": (demod_input, run_demod), "descramble": (descramble_input, run_descramble),
    "encode": (encode_input, run_encode), "rate_match": (rate_match_input, run_rate_match),
}


def input_digest(inp) -> str:
    return digest(*inp) if isinstance(inp, tuple) else digest(inp)


GOLDEN = Path(__file__).resolve().parent / "golden"


def load_fixture(op):
    """(cases, recorded reference outputs, inputs) of tests/golden/ref_<op>.npz. Inputs are regenerated from the seeds
    (stored ones are read) and every input's SHA-256 must equal the recorded one: a mismatch is an AssertionError."""
    cases, outs, stored = unpack_fixture(np.load(GOLDEN / f"ref_{op}.npz", allow_pickle=False))
    inputs = stored if stored is not None else [OPS[op][0](c) for c in cases]
    for c, inp in zip(cases, inputs):
        assert input_digest(inp) == c["sha"], f"ref_{op}.npz: the regenerated input of {c} has another digest"
    return cases, outs, inputs
