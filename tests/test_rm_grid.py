"""CPU tests of the rate matcher's branch grid itself (tests/rm_grid.py): the conditions the GPU comparison
(tests/test_gpu_rm_grid.py) relies on. Every input is one the reference accepts, every label of rm_trace is reached on
every branch graph, every named row is what its name says, the oracle accepts every case, no device route drops a row,
and rm_trace agrees with what the oracle selects from a codeword whose bits are tagged with their positions."""
import numpy as np
import pytest

import oracle as O
from tests import ref_cases as C
from tests import rm_grid as G

GRID = G.grid_cases()
ROWS = G.all_rows()
NBRANCH = 20


def _of(bg, Z, kind="branch", cases=ROWS):
    return [c for c in cases if (c["bg"], c["Z"], c["kind"]) == (bg, Z, kind)]


def _geo(c):
    return G.geometry(c["bg"], c["Z"], c["rv"], c["F"], c["Nref"])


def test_grid_shape():
    assert len(GRID) == NBRANCH * len(G.BRANCH_GRAPHS) + len(C.GRAPHS) == 342
    assert len(G.STAGING_ROWS) == len(G.STAGING_E) * len(G.WIDTH_GRAPHS) + 4 + 2 * len(G.QMS) == 66
    assert len({c["seed"] for c in ROWS}) == len(ROWS)
    for bg, Z in G.BRANCH_GRAPHS:
        assert len(_of(bg, Z)) == NBRANCH and len({c["row"] for c in _of(bg, Z)}) == NBRANCH
    every = [c for c in GRID if c["kind"] == "graph"]
    assert [(c["bg"], c["Z"]) for c in every] == C.GRAPHS and len(every) == 102
    assert {c["rv"] for c in every} == {0, 1, 2, 3} and {c["Qm"] for c in every} == set(G.QMS)
    for c in every:
        g = _geo(c)
        assert g["lap"] + 1 <= c["E"] < g["lap"] + 1 + c["Qm"] and c["Nref"] == 0
        assert c["F"] == (C.filler_of(c["Z"]) if C.filler_of(c["Z"]) < g["nsys"] else 0)
        assert {"wrap", "laps2"} <= G.trace_of(c)
    assert sum(c["F"] > 0 for c in every) >= 98


def test_inputs_are_legal():
    for c in ROWS:
        g = _geo(c)
        assert c["E"] > 0 and c["E"] % c["Qm"] == 0 and c["Qm"] in G.QMS and 0 <= c["rv"] <= 3, c
        assert c["F"] < g["nsys"] and g["Ncb"] >= g["nsys"] + 1, c
        assert (c["E"] <= G.MAX_CODEBLOCK_RM_SIZE) == (c["kind"] != "division"), c
        msg = C.rm_message(c)
        assert msg.size == O.BG_K[c["bg"]] * c["Z"] and np.all(msg[:msg.size - c["F"]] <= 1)
        assert np.all(msg[msg.size - c["F"]:] == O.FILLER_BIT)
    assert all(c["kind"] != "division" for c in G.reference_rows()) and len(G.reference_rows()) == len(ROWS) - 4


@pytest.mark.parametrize("bg,Z", G.BRANCH_GRAPHS)
def test_every_label_on_every_graph(bg, Z):
    """Per graph, not over the union."""
    got = set().union(*[G.trace_of(c) for c in _of(bg, Z)])
    print(f"BG{bg} Z={Z}: {len(got & G.LABELS)} of {len(G.LABELS)} labels")
    assert got >= G.LABELS, sorted(G.LABELS - got)


def test_rows_are_what_their_names_say():
    for bg, Z in G.BRANCH_GRAPHS:
        r = {c["row"]: c for c in _of(bg, Z)}
        E = {k: c["E"] for k, c in r.items()}
        g = {k: _geo(c) for k, c in r.items()}
        t = {k: G.trace_of(c) for k, c in r.items()}
        for k in r:
            assert g[k]["ninfo"] == g[k]["nsys"] - r[k]["F"]           # fl
        assert E["ends_at_fl_minus_1_exact"] == g["ends_at_fl_minus_1_exact"]["ninfo"] and r[
            "ends_at_fl_minus_1_exact"]["F"] > 0 and "ends_at_fl_minus_1" in t["ends_at_fl_minus_1_exact"]
        k = "one_symbol_past_gap"
        assert g[k]["ninfo"] + 1 <= E[k] < g[k]["ninfo"] + 1 + r[k]["Qm"] and "crosses_gap" in t[k]
        assert E["one_lap_exact"] == g["one_lap_exact"]["lap"] == g["one_lap_exact"]["N"]
        assert {"end_at_ncb_exact", "laps1", "no_fillers", "k0_zero"} <= t["one_lap_exact"]
        assert E["one_lap_plus_1_exact"] == g["one_lap_plus_1_exact"]["lap"] + 1
        assert {"wrap", "laps2", "crosses_gap", "end_before_ncb"} <= t["one_lap_plus_1_exact"]
        assert E["two_laps_exact"] == 2 * g["two_laps_exact"]["lap"]
        assert {"wrap", "laps2", "end_at_ncb_exact"} <= t["two_laps_exact"]
        assert E["multi_lap"] >= 2 * g["multi_lap"]["lap"] and "laps3plus" in t["multi_lap"]
        k = "k0_info_short"
        assert 0 < g[k]["k0"] < g[k]["ninfo"] and "k0_info" in t[k]
        k = "k0_in_fillers"
        assert g[k]["ninfo"] < g[k]["k0"] < g[k]["nsys"] and {"k0_in_fillers", "starts_after_gap"} <= t[k]
        k = "k0_at_fl_lap_plus_1_exact"
        assert g[k]["k0"] == g[k]["ninfo"] < g[k]["nsys"] and E[k] == g[k]["lap"] + 1 and "k0_at_fl" in t[k]
        k = "k0_at_fh_to_end_exact"
        assert g[k]["k0"] == g[k]["nsys"] and r[k]["F"] > 0 and E[k] == g[k]["Ncb"] - g[k]["k0"]
        assert {"k0_at_fh", "end_at_ncb_exact", "laps1", "lbrm"} <= t[k]
        k = "rv2_to_end_exact"
        assert E[k] == g[k]["Ncb"] - g[k]["k0"] and {"k0_parity", "end_at_ncb_exact", "laps1"} <= t[k]
        k = "rv3_to_end_plus_1_exact"
        assert E[k] == g[k]["Ncb"] - g[k]["k0"] + 1 and {"k0_parity", "wrap", "laps2"} <= t[k]
        for k in ("lbrm_min_rv3", "lbrm_min_multi_lap"):
            assert g[k]["Ncb"] == g[k]["nsys"] + 1 and "lbrm_min" in t[k]
        assert "laps3plus" in t["lbrm_min_multi_lap"]
        k = "lbrm_n_minus_1_lap_exact"
        assert g[k]["Ncb"] == g[k]["N"] - 1 == E[k] and {"lbrm", "wrap"} <= t[k]
        k = "lbrm_mid_to_end_plus_1_exact"
        assert E[k] == g[k]["Ncb"] - g[k]["k0"] + 1 and g[k]["nsys"] + 1 < g[k]["Ncb"] < g[k]["N"]
        k = "nref_above_n_short"
        assert r[k]["Nref"] > g[k]["N"] == g[k]["Ncb"] and "nref_above_n" in t[k]
        assert E["one_symbol"] == r["one_symbol"]["Qm"] == 8 and E["one_bit"] == r["one_bit"]["Qm"] == 1
        assert "eq1" in t["one_symbol"] and "eq1" in t["one_bit"]


def test_staging_rows_are_what_their_names_say():
    for bg, Z in G.WIDTH_GRAPHS:
        rows = _of(bg, Z, "staging")
        assert [c["row"] for c in rows] == [f"e_{t}" for t in G.STAGING_E]
        assert {c["Qm"] for c in rows} == set(G.QMS) and {c["rv"] for c in rows} == {0, 1, 2, 3}
        for c, t in zip(rows, G.STAGING_E):
            assert abs(c["E"] - t) <= max(c["Qm"] // 2, c["Qm"] - t) and c["E"] <= G.MAX_CODEBLOCK_RM_SIZE, c
        E = {c["row"]: c["E"] for c in rows}
        assert E[f"e_{G.MAX_CODEBLOCK_RM_SIZE}"] == G.MAX_CODEBLOCK_RM_SIZE
        # pdsch_rate_match stages 32768 bits per chunk: one chunk, exactly one, a second one of 8 bits or less
        assert E["e_32760"] <= 32768 - 4 and E["e_32768"] in (32766, 32768, 32770) and 32768 < E["e_32776"]
        last = E["e_65576"] - 2 * 32768          # the third chunk: fewer than 16 bytes, so no 16-byte store at all
        assert 0 < (last + 7) // 8 < 16
        last = (E["e_106307"] - 3 * 32768 + 7) // 8
        assert last >= 16 and last % 16 != 0     # 16-byte stores and a byte tail
    # over the four graphs every staging length meets at least four modulation orders
    for t in G.STAGING_E:
        assert len({c["Qm"] for c in G.STAGING_ROWS if c["row"] == f"e_{t}"}) == 4
    div = [c for c in G.STAGING_ROWS if c["kind"] == "division"]
    assert [(c["bg"], c["Z"]) for c in div] == [(2, 2), (2, 2), (1, 384), (1, 384)]
    for c in div:
        g = _geo(c)
        r0 = g["k0"]                             # F = 0 and k0 below the systematic bits' end or not: rank = position
        assert c["F"] == 0 and c["Nref"] == 0
        assert r0 + c["E"] == (G.DIVISION_LIMIT - c["Qm"] if c["row"] == "below_2^21" else G.DIVISION_LIMIT)
    assert {_geo(c)["k0"] for c in div} == {0, 17 * 384}
    wrap = [c for c in G.STAGING_ROWS if c["kind"] == "wrap"]
    assert [c["Qm"] for c in wrap] == [q for q in G.QMS for _ in (0, 1)]
    for c in wrap:
        g, nsc = _geo(c), G.MOD_CHUNK_SYMS[c["Qm"]]
        L, EQ = g["lap"], c["E"] // c["Qm"]
        assert g["k0"] == 0 and EQ > L + nsc                      # bit 0 of symbol s has rank s: the wrap is reached
        at = (L - 1) % nsc                                        # the place in its chunk of the symbol with r + 1 == L
        assert at == (0 if c["row"] == "wrap_on_chunk_start" else nsc // 2) and 0 < nsc // 2 < nsc - 1


def test_no_route_drops_a_row():
    """route_skip is the one place a device route may leave a row out; the counts are asserted here so that no rule
    can hide a failure. Every route keeps every branch row and all 102 every-graph rows."""
    for route in G.ROUTES:
        dropped = [c for c in ROWS if G.route_skip(route, c) is not None]
        print(f"{route}: {len(dropped)} of {len(ROWS)} rows dropped")
        assert len(dropped) == 0
        kept = [c for c in ROWS if G.route_skip(route, c) is None]
        assert sum(c["kind"] == "branch" for c in kept) == NBRANCH * len(G.BRANCH_GRAPHS)
        assert sum(c["kind"] == "graph" for c in kept) == 102


def test_fused_encoder_batches_stay_on_their_route():
    """The batches tests/pdsch_flow.encode_cbs makes in each context of the fused encoder (plan_batches restates its
    rule): where the context is about a zero-copy route every batch stages at most the 1 MiB up to which the queue
    stays zero-copy, the work queue's batches hold at most 8 codeblocks, and the exact-division rows (r0 + E = 2^21) sit
    in such batches; without the limit the last batch of 162 would stage more and be copied, which is what the copy
    context runs on purpose."""
    from tests.pdsch_flow import ENC_DWQ_MAX_CBS, ENC_ZERO_COPY_MAX_BYTES, cb_staged_bytes, plan_batches
    for name, (flags, max_cbs, max_bytes, kinds) in G.ENC_CONTEXTS.items():
        rows = [c for c in ROWS if kinds is None or c["kind"] in kinds]
        plan = plan_batches(rows, max_cbs, max_bytes)
        assert [a for a, _ in plan] == [0] + [b for _, b in plan[:-1]] and plan[-1][1] == len(rows)
        sizes = [sum(cb_staged_bytes(c) for c in rows[a:b]) for a, b in plan]
        print(f"{name}: {len(plan)} batches, largest {max(sizes)} bytes")
        assert all(b - a <= (max_cbs or 162) for a, b in plan)
        if "LAUNCH_HAL_COPY" in flags:
            assert max_bytes is None and max(sizes) > ENC_ZERO_COPY_MAX_BYTES
            continue
        assert max_bytes == ENC_ZERO_COPY_MAX_BYTES and max(sizes) <= ENC_ZERO_COPY_MAX_BYTES
        if "LAUNCH_NO_DWQ" not in flags:
            assert max_cbs == ENC_DWQ_MAX_CBS
        if max_cbs == 0:
            assert any(b - a > 1 and any(c["kind"] == "division" for c in rows[a:b]) for a, b in plan)
        assert sum(c["row"] == "at_2^21" for c in rows) == 2
    assert len(plan_batches(ROWS, 0, None)) == 3 and len(plan_batches(ROWS, 0, 1 << 20)) == 4
    assert len(plan_batches(ROWS, 8, 1 << 20)) == 52 and len(plan_batches(ROWS, 8, None)) == 51


def test_oracle_accepts_every_case():
    """Without raising; the selected bits hold no filler marker."""
    for c in ROWS:
        cw = C.rate_match_input(c)
        g = _geo(c)
        assert np.all(cw[g["ninfo"]:g["nsys"]] == O.FILLER_BIT) and np.count_nonzero(cw == O.FILLER_BIT) == c["F"]
        out = O.rate_match(cw, c["E"], c["rv"], c["Qm"], c["Nref"], c["bg"], c["Z"])
        assert out.size == c["E"] and np.all(out <= 1), c


def _selected_positions(c):
    """The codeword positions the oracle selects, in selection order: the oracle runs once per bit b of the position
    index on a 'codeword' whose bit p is bit b of p (filler markers kept), and the interleaver is undone."""
    g = _geo(c)
    N, E, Qm = g["N"], c["E"], c["Qm"]
    p = np.arange(N)
    pos = np.zeros(E, np.int64)
    for b in range(int(N - 1).bit_length()):
        cw = ((p >> b) & 1).astype(np.uint8)
        cw[g["ninfo"]:g["nsys"]] = O.FILLER_BIT
        out = O.rate_match(cw, E, c["rv"], Qm, c["Nref"], c["bg"], c["Z"])
        # selected bit i EQ + jj is output bit jj Qm + i
        pos |= out.reshape(E // Qm, Qm).T.reshape(-1).astype(np.int64) << b
    return pos


@pytest.mark.parametrize("bg,Z", G.BRANCH_GRAPHS)
def test_trace_agrees_with_the_oracle_on_tagged_codewords(bg, Z):
    """Holds rm_trace to the oracle independently of itself: first and last selected position, number of wraps,
    whether fl - 1 -> fh occurs, and that the selection is the circular walk without the filler range."""
    for c in _of(bg, Z) + [x for x in _of(bg, Z, "graph")]:
        g, t = _geo(c), G.trace_of(c)
        fl, fh, Ncb, k0 = g["ninfo"], g["nsys"], g["Ncb"], g["k0"]
        pos = _selected_positions(c)
        assert np.all((pos < fl) | (pos >= fh)) and np.all(pos < Ncb), c
        step = np.diff(pos)
        nxt = np.where(pos[:-1] == fl - 1, fh, pos[:-1] + 1) if c["F"] else pos[:-1] + 1
        assert np.array_equal(pos[1:], np.where(nxt == Ncb, 0, nxt)), c
        start = {s for s in ("k0_zero", "k0_info", "k0_at_fl", "k0_in_fillers", "k0_at_fh", "k0_parity") if s in t}
        assert len(start) == 1, c
        s = start.pop()
        first = int(pos[0])
        assert {"k0_zero": first == 0, "k0_info": first == k0 and 0 < first < fl,
                "k0_at_fl": first == fh and k0 == fl and c["F"] > 0,
                "k0_in_fillers": first == fh and fl < k0 < fh, "k0_at_fh": first == fh == k0,
                "k0_parity": first == k0 > fh}[s], (c, s, first)
        assert ("starts_after_gap" in t) == (first >= fh), c
        last = int(pos[-1])
        assert ("end_at_ncb_exact" in t) == (last == Ncb - 1) and ("end_before_ncb" in t) == (last < Ncb - 1), c
        assert ("ends_at_fl_minus_1" in t) == (c["F"] > 0 and last == fl - 1), c
        wraps = int(np.count_nonzero(step < 0))
        assert ("wrap" in t) == (wraps > 0), c
        assert f"laps{wraps + 1}" in t if wraps < 2 else "laps3plus" in t, (c, wraps)
        crosses = bool(c["F"]) and bool(np.any((pos[:-1] == fl - 1) & (pos[1:] == fh)))
        assert ("crosses_gap" in t) == crosses, c
