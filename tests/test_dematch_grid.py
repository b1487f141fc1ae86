"""CPU tests of the dematcher's branch grid itself (tests/dematch_grid.py): the conditions the GPU comparison
(tests/test_gpu_dematch_grid.py) relies on. The oracle accepts every case, every label of allot_trace is reached on
every graph, the symbol and scrambled forms keep all but the over-long and the empty rows, and every input is one the
reference accepts. Plus the oracle's refusal of a limited buffer shorter than the systematic bits."""
import numpy as np
import pytest

import oracle as O
from tests import dematch_grid as G
from tests import ref_cases as C

CASES = G.grid_cases()
ALL = G.LABELS | G.EXTRA_LABELS


def _of(bg, Z, kind="branch", cases=CASES):
    return [c for c in cases if (c["bg"], c["Z"], c["kind"]) == (bg, Z, kind)]


def test_grid_shape():
    assert len(CASES) == 19 * len(G.BRANCH_GRAPHS) + len(G.WIDTH_EQ) * len(G.WIDTH_GRAPHS) == 300
    assert len({c["seed"] for c in CASES}) == len(CASES)
    for bg, Z in G.BRANCH_GRAPHS:
        assert len(_of(bg, Z)) == 19 and len({c["row"] for c in _of(bg, Z)}) == 19
    for bg, Z in G.WIDTH_GRAPHS:
        rows = _of(bg, Z, "width")
        assert [c["E"] // c["Qm"] for c in rows] == G.WIDTH_EQ
        assert {c["Qm"] for c in rows} == set(G.QMS)
        assert all((c["rv"], c["F"], c["Nref"]) == (0, 0, 0) for c in rows)


def test_width_rows_straddle_every_workgroup_width():
    """For every width a decode kernel can have (64 .. 1024 in whole waves), both dq = 0 and dq >= 1 and both dr = 0 and
    dr != 0 occur among the E / Qm values, and E / Qm = width - 1, width, width + 1 for the power-of-two widths."""
    eqs = set(G.WIDTH_EQ)
    for nth in range(64, 1025, 64):
        dq = {nth // eq for eq in eqs}
        dr = {nth % eq for eq in eqs}
        assert 0 in dq and any(q >= 1 for q in dq) and 0 in dr and any(r != 0 for r in dr), nth
    for nth in (64, 128, 256, 512, 1024):
        assert {nth - 1, nth, nth + 1} <= eqs


def test_inputs_are_legal():
    for c in CASES:
        g = G.geometry(c["bg"], c["Z"], c["rv"], c["F"], c["Nref"])
        assert c["E"] % c["Qm"] == 0 and c["Qm"] in G.QMS and 0 <= c["rv"] <= 3, c
        assert c["F"] < g["nsys"] and g["Ncb"] >= g["nsys"] and c["Nref"] <= 66 * 384, c
        assert c["E"] <= G.MAX_CODEBLOCK_RM_SIZE, c
        for v in C.dematch_input(c):
            a = np.abs(v.astype(np.int16))
            assert np.all((a <= 120) | (a == 127)), c


def test_rows_are_what_their_names_say():
    for bg, Z in G.BRANCH_GRAPHS:
        r = {c["row"]: c for c in _of(bg, Z)}

        def geo(name):
            c = r[name]
            return G.geometry(bg, Z, c["rv"], c["F"], c["Nref"])
        assert r["end_in_info"]["E"] == geo("end_in_info")["ninfo"] - 1
        assert r["end_at_ninfo_exact"]["E"] == geo("end_at_ninfo_exact")["ninfo"]
        assert r["one_lap_exact"]["E"] == geo("one_lap_exact")["lap"]
        assert r["one_lap_plus_1_exact"]["E"] == geo("one_lap_plus_1_exact")["lap"] + 1
        g = geo("k0_in_fillers")
        assert g["ninfo"] < g["k0"] < g["nsys"]
        g = geo("k0_at_ninfo_exact")
        assert g["k0"] == g["ninfo"] and r["k0_at_ninfo_exact"]["E"] == g["lap"] + 1
        g = geo("rv2_to_end_exact")
        assert r["rv2_to_end_exact"]["E"] == g["Ncb"] - g["k0"]
        g = geo("rv3_to_end_plus_1_exact")
        assert r["rv3_to_end_plus_1_exact"]["E"] == g["Ncb"] - g["k0"] + 1
        g = geo("lbrm_mid_to_end_plus_1_exact")
        assert r["lbrm_mid_to_end_plus_1_exact"]["E"] == g["Ncb"] - g["k0"] + 1 and g["Ncb"] < g["N"]
        assert geo("lbrm_min_rv3")["Ncb"] == geo("lbrm_min_rv3")["nsys"] + 1
        assert geo("nref_above_n_one_llr")["Ncb"] == geo("nref_above_n_one_llr")["N"]
        assert r["empty"]["E"] == 0 and r["multi_lap"]["E"] >= 2 * geo("multi_lap")["lap"]


@pytest.mark.parametrize("bg,Z", G.BRANCH_GRAPHS)
def test_every_label_on_every_graph(bg, Z):
    """Per graph, not over the union: BG2 too, thanks to the limited-buffer variant of its two filler rows."""
    got = set().union(*[G.labels_of(c) for c in _of(bg, Z)])
    assert got >= ALL, sorted(ALL - got)
    assert set().union(*[G.trace_of(c, True) for c in _of(bg, Z)]) >= {"tail_zero", "tail_zero_lbrm", "no_tail"}


def test_labels_in_the_symbol_and_scrambled_forms():
    """Those forms keep the rows that fit the LDS staging and hold a symbol (fits_staging, the one rule). Over the union
    of graphs they reach every label but passes0 (the empty row's own); per graph every label except those whose only
    row is left out; at least 17 of the 19 rows of every graph stay, and only the multi-lap row at Z >= 256 and the
    empty row fall out."""
    kept = [c for c in CASES if G.fits_staging(c)]
    assert set().union(*[G.labels_of(c) for c in kept]) >= ALL - {"passes0"}
    for bg, Z in G.BRANCH_GRAPHS:
        rows = _of(bg, Z)
        stay = [c for c in rows if G.fits_staging(c)]
        out = [c for c in rows if not G.fits_staging(c)]
        assert len(stay) >= 17
        assert {c["row"] for c in out} <= {"multi_lap", "empty"} and (Z >= 256 or len(out) == 1)
        only_out = set().union(*[G.labels_of(c) for c in out]) - set().union(*[G.labels_of(c) for c in stay])
        assert set().union(*[G.labels_of(c) for c in stay]) >= ALL - only_out
        assert only_out <= {"passes0"}, only_out  # passes3 survives through the limited buffer's multi-lap row
    assert all(G.fits_staging(c) for c in CASES if c["kind"] == "width")


def test_oracle_accepts_every_case():
    """New data and combine, without raising; fillers read +127 after a new-data pass."""
    for c in CASES:
        res = C.run_dematch(C.ORACLE, c, C.dematch_input(c))
        g = G.geometry(c["bg"], c["Z"], c["rv"], c["F"], c["Nref"])
        if c["E"]:
            assert np.all(res["soft_new"][g["ninfo"]:g["nsys"]] == 127), c


@pytest.mark.parametrize("bg,Z", [(1, 2), (2, 3), (1, 384), (2, 384)])
def test_oracle_refuses_a_buffer_shorter_than_the_systematic_bits(bg, Z):
    """Ncb = (K - 2) Z - 1 raises and leaves the buffer alone (buffer_length - tmp_idx would wrap and the copy run past
    the codeblock); Ncb = (K - 2) Z is the legal edge: an empty parity range."""
    N, nsys = O.BG_N_SHORT[bg] * Z, (O.BG_K[bg] - 2) * Z
    tx = np.full(2 * Z + 6, 7, np.int8)
    for new_data in (True, False):
        soft = np.full(N, 33, np.int8)
        with pytest.raises(ValueError):
            O.rate_dematch(soft, tx, new_data, 0, 2, nsys - 1, 0)
        assert np.all(soft == 33)
    soft = np.full(N, 33, np.int8)
    O.rate_dematch(soft, tx, True, 0, 2, nsys, 0)
    # tmp_idx is raised to nsys and wraps to 0 there, so no tail is zeroed: only the copied LLRs change
    assert np.all(soft[:tx.size] == 7) and np.all(soft[tx.size:] == 33)
