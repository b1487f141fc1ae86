"""The rate matcher's branch grid: cases that reach every branch of select_bits and interleave_bits
(ldpc_rate_matcher_impl.cpp:36-160) on graphs of every encoder layout, every lifted graph once, and E around every
staging boundary of the fused encoder's rate matcher (csrc/ldpc_downlink_kernels.hip pdsch_rate_match).
tests/test_rm_grid.py checks the grid's own conditions on the CPU, tests/ref_cases.live_rate_match_cases() and
tests/golden/ref_rate_match_grid.json hold the oracle to the reference on it, and tests/test_gpu_rm_grid.py holds the
three device rate matchers (ldpc_rate_match_kernel, pdsch_rate_match, mod_rate_match) to the oracle on it.

A case is tests/ref_cases.rate_match_cases' dict of plain numbers plus the name of its row and its kind; its input is
tests/ref_cases.rate_match_input's: the codeword O.ldpc_encode gives for the seeded message (rm_message), fillers at
the message tail, so at codeword bits [fl, fh) = [nsys - F, nsys).

rm_trace() restates the control flow only (it moves no data) and names what a case reaches:

  start        k0_zero, k0_info (0 < k0 < fl), k0_at_fl (F > 0: jumps to fh), k0_in_fillers (fl < k0 < fh: jumps to
               fh), k0_at_fh, k0_parity (k0 > fh)
  gap          no_fillers (F = 0), crosses_gap (F > 0: selects bit fl - 1 and then bit fh), ends_at_fl_minus_1 (F > 0:
               the last selected bit is fl - 1), starts_after_gap (the first selected bit is at or above fh)
  end          end_before_ncb (the last selected bit is below Ncb - 1), end_at_ncb_exact (it is Ncb - 1), wrap (the
               selection goes on at bit 0), laps1 / laps2 / laps3plus (the buffer's end is passed 0 / 1 / 2 or more
               times: wraps + 1)
  buffer       full_buffer (Nref = 0), lbrm (Ncb < N), lbrm_min (Ncb = nsys + 1), nref_above_n (Nref > N)
  interleaver  qm1, qm2, qm4, qm6, qm8, eq1 (E = Qm: one symbol)

A buffer cut inside the systematic bits (Ncb <= nsys) is not something the reference defines; no row has one.

The staging rows (STAGING_ROWS) only matter to the device: pdsch_rate_match produces 256 bits per round, stages
ENC_OBUF = 4096 bytes (32768 bits) per chunk and stores a chunk in 16-byte pieces with a byte tail; it divides by a
float reciprocal while r0 + E < 2^21 and exactly above (the 'division' rows, which the reference, limited to
MAX_CODEBLOCK_RM_SIZE, does not take); mod_rate_match gives one thread a chunk of mod_chunk_syms symbols (32, 16, 8, 16,
4 for Qm 1, 2, 4, 6, 8) and steps through the circular buffer with a wrap test per symbol (the 'wrap' rows put that
wrap inside a chunk and on a chunk's first symbol)."""
from __future__ import annotations

import oracle as O
from tests.dematch_grid import BRANCH_GRAPHS, MAX_CODEBLOCK_RM_SIZE, QMS, WIDTH_GRAPHS, geometry, qm_dividing, up
from tests.ref_cases import GRAPHS, filler_of

LABELS = frozenset("""k0_zero k0_info k0_at_fl k0_in_fillers k0_at_fh k0_parity no_fillers crosses_gap
ends_at_fl_minus_1 starts_after_gap end_before_ncb end_at_ncb_exact wrap laps1 laps2 laps3plus full_buffer lbrm
lbrm_min nref_above_n qm1 qm2 qm4 qm6 qm8 eq1""".split())
STAGING_E = [8, 64, 255, 256, 257, 2047, 2048, 32768 - 8, 32768, 32768 + 8, 2 * 32768 + 40, 3 * 32768 + 8 * 1000 + 3,
             MAX_CODEBLOCK_RM_SIZE]
DIVISION_LIMIT = 1 << 21                       # pdsch_rate_match: fast = r0 + E < 2^21
MOD_CHUNK_SYMS = {1: 32, 2: 16, 4: 8, 6: 16, 8: 4}  # csrc/ldpc_modulation_kernels.hip mod_chunk_syms
WRAP_GRAPH = (2, 36)


def rm_trace(bg, Z, E, rv, Qm, F, Nref) -> set:
    """The labels (module docstring) select_bits and interleave_bits reach for this case."""
    g = geometry(bg, Z, rv, F, Nref)
    N, nsys, fl, Ncb, k0 = g["N"], g["nsys"], g["ninfo"], g["Ncb"], g["k0"]
    fh = nsys
    assert E > 0 and E % Qm == 0 and F < nsys and Ncb >= nsys + 1
    got = {f"qm{Qm}"}
    if E == Qm:
        got.add("eq1")
    got.add("full_buffer" if Nref == 0 else "lbrm" if Ncb < N else "nref_above_n" if Nref > N else "nref_eq_n")
    assert "nref_eq_n" not in got, "no row has Nref = N: it would be one more spelling of the full buffer"
    if Ncb == nsys + 1:
        got.add("lbrm_min")
    if F == 0:
        got.add("no_fillers")
    got.add("k0_zero" if k0 == 0 else "k0_info" if k0 < fl else "k0_at_fl" if k0 == fl and F > 0
            else "k0_in_fillers" if k0 < fh else "k0_at_fh" if k0 == fh else "k0_parity")
    out, idx, wraps, first, last = 0, k0, 0, None, None
    while out < E:
        if fl <= idx < fh:
            idx = fh
        if first is None:
            first = idx
            if first >= fh:
                got.add("starts_after_gap")
        stop = fl if (F > 0 and idx <= fl) else Ncb
        count = min(stop - idx, E - out)
        out += count
        last = idx + count - 1
        if F > 0 and last == fl - 1:
            got.add("crosses_gap" if out < E else "ends_at_fl_minus_1")
        if idx + count == Ncb and out < E:
            got.add("wrap")
            wraps += 1
        idx = (idx + count) % Ncb
    got.add("end_at_ncb_exact" if last == Ncb - 1 else "end_before_ncb")
    got.add(f"laps{wraps + 1}" if wraps < 2 else "laps3plus")
    return got


def branch_rows(bg, Z):
    """20 (name, Qm, rv, F, Nref, E) rows built from the graph's own fl, nsys, Ncb, k0 and lap = Ncb - F. E is rounded
    up to a multiple of Qm, except in the rows named 'exact', which take the largest modulation order up to the row's
    that divides the length they are about. On BG2 rv 1 starts in the parity part of an unlimited buffer, so the rows
    that put k0 below, at and inside the filler range limit the buffer to nsys + 1 there (k0 = 2 Z); with Nref = 2 nsys
    rv 2 starts exactly at fh on both base graphs."""
    N, nsys = O.BG_N_SHORT[bg] * Z, (O.BG_K[bg] - 2) * Z
    Fh, mid = Z // 2 + 1, (nsys + N) // 2 + 3
    fill_nref = 0 if bg == 1 else nsys + 1

    def g(rv=0, F=0, Nref=0):
        return geometry(bg, Z, rv, F, Nref)

    k0f = g(1, 0, fill_nref)["k0"]  # k0 does not depend on F
    assert 5 < k0f < nsys - Fh and g(2, 0, 2 * nsys)["k0"] == nsys
    rows = [
        ("ends_at_fl_minus_1_exact", 8, 0, Fh, 0, nsys - Fh, True),
        ("one_symbol_past_gap", 4, 0, Fh, 0, nsys - Fh + 1, False),
        ("one_lap_exact", 6, 0, 0, 0, g()["lap"], True),
        ("one_lap_plus_1_exact", 8, 0, Fh, 0, g(0, Fh)["lap"] + 1, True),
        ("two_laps_exact", 4, 0, Fh, 0, 2 * g(0, Fh)["lap"], True),
        ("multi_lap", 8, 0, 0, 0, 2 * N + N // 3, False),
        ("k0_info_short", 6, 1, Fh, fill_nref, Z + 3, False),
        ("k0_in_fillers", 4, 1, nsys - k0f + 5, fill_nref, Z + 3, False),
        ("k0_at_fl_lap_plus_1_exact", 2, 1, nsys - k0f, fill_nref, g(1, nsys - k0f, fill_nref)["lap"] + 1, True),
        ("k0_at_fh_to_end_exact", 8, 2, Fh, 2 * nsys, 2 * nsys - nsys, True),
        ("rv2_fillers_short", 1, 2, Fh, 0, Z + 3, False),
        ("rv2_to_end_exact", 6, 2, 0, 0, N - g(2)["k0"], True),
        ("rv3_to_end_plus_1_exact", 4, 3, 0, 0, N - g(3)["k0"] + 1, True),
        ("lbrm_min_rv3", 2, 3, Fh, nsys + 1, Z + 3, False),
        ("lbrm_min_multi_lap", 6, 2, Fh, nsys + 1, 3 * (nsys + 1 - Fh) + (nsys + 1) // 3, False),
        ("lbrm_n_minus_1_lap_exact", 8, 3, 0, N - 1, N - 1, True),
        ("lbrm_mid_to_end_plus_1_exact", 1, 3, Fh, mid, mid - g(3, Fh, mid)["k0"] + 1, True),
        ("nref_above_n_short", 2, 1, 0, N + 5, Z + 3, False),
        ("one_symbol", 8, 1, 0, mid, 8, True),
        ("one_bit", 1, 0, Fh, 0, 1, True),
    ]
    out = []
    for name, Qm, rv, F, Nref, E, exact in rows:
        if exact:
            Qm = qm_dividing(E, Qm)
        out.append((name, Qm, rv, F, Nref, up(E, Qm)))
    return out


def _case(bg, Z, E, rv, Qm, F, Nref, seed, row, kind):
    return dict(bg=bg, Z=Z, E=E, rv=rv, Qm=Qm, Nref=Nref, F=F, seed=seed, row=row, kind=kind)


def grid_cases():
    """The branch rows of BRANCH_GRAPHS (seeds 72000 + i), then one row per lifted graph (seeds 73000 + g): F =
    filler_of(Z) where it fits below the systematic bits, rv and Qm rotating, E = lap + 1 rounded up to Qm, so every
    selectable bit of every codeword column is read once and the wrap is taken."""
    cases = []
    for bg, Z in BRANCH_GRAPHS:
        for name, Qm, rv, F, Nref, E in branch_rows(bg, Z):
            cases.append(_case(bg, Z, E, rv, Qm, F, Nref, 72000 + len(cases), name, "branch"))
    for g, (bg, Z) in enumerate(GRAPHS):
        F = filler_of(Z) if filler_of(Z) < (O.BG_K[bg] - 2) * Z else 0
        rv, Qm = g % 4, QMS[g % 5]
        E = up(geometry(bg, Z, rv, F, 0)["lap"] + 1, Qm)
        cases.append(_case(bg, Z, E, rv, Qm, F, 0, 73000 + g, "every_graph", "graph"))
    return cases


def _nearest(E, Qm):
    return max(Qm, (E + Qm // 2) // Qm * Qm)


def _staging_rows():
    """'staging': on WIDTH_GRAPHS, E the multiple of Qm nearest to every STAGING_E value (not above the last), Qm, rv
    and the filler count rotating. 'division': r0 + E = 2^21 - Qm (the largest operands of the reciprocal division) and
    2^21 (the exact division), with r0 = 0 on (2, 2) and r0 = k0 = 17 Z on (1, 384). 'wrap': per Qm, on WRAP_GRAPH with
    rv 0, F chosen so that L = N - F puts rank L - 1 (mod_rate_match's r + 1 == L) in the middle of a thread's chunk
    and on a chunk's first symbol; E = (L + chunk + 3) Qm."""
    rows = []

    def add(bg, Z, E, rv, Qm, F, Nref, row, kind):
        rows.append(_case(bg, Z, E, rv, Qm, F, Nref, 74000 + len(rows), row, kind))

    for gi, (bg, Z) in enumerate(WIDTH_GRAPHS):
        for i, target in enumerate(STAGING_E):
            Qm = QMS[(i + gi) % 5]
            E = min(_nearest(target, Qm), MAX_CODEBLOCK_RM_SIZE // Qm * Qm)
            F = filler_of(Z) if (i % 2 and filler_of(Z) < (O.BG_K[bg] - 2) * Z) else 0
            add(bg, Z, E, (i + gi) % 4, Qm, F, 0, f"e_{target}", "staging")
    for (bg, Z), rv, qms in (((2, 2), 0, (8, 2)), ((1, 384), 1, (8, 4))):
        r0 = geometry(bg, Z, rv, 0, 0)["k0"]
        add(bg, Z, DIVISION_LIMIT - r0 - qms[0], rv, qms[0], 0, 0, "below_2^21", "division")
        add(bg, Z, DIVISION_LIMIT - r0, rv, qms[1], 0, 0, "at_2^21", "division")
    bg, Z = WRAP_GRAPH
    N = O.BG_N_SHORT[bg] * Z
    for Qm in QMS:
        nsc = MOD_CHUNK_SYMS[Qm]
        for row, at in (("wrap_inside_chunk", nsc // 2), ("wrap_on_chunk_start", 0)):
            F = (N - 1 - at) % nsc
            add(bg, Z, (N - F + nsc + 3) * Qm, 0, Qm, F, 0, row, "wrap")
    return rows


STAGING_ROWS = _staging_rows()


def all_rows():
    """What every device route runs: the grid, then STAGING_ROWS."""
    return grid_cases() + STAGING_ROWS


def reference_rows():
    """What the compiled reference takes: everything but the 'division' rows (E above MAX_CODEBLOCK_RM_SIZE)."""
    return [c for c in all_rows() if c["kind"] != "division"]


def trace_of(c):
    return rm_trace(c["bg"], c["Z"], c["E"], c["rv"], c["Qm"], c["F"], c["Nref"])


ROUTES = ("rate_match_launch", "pdsch_encode", "rate_match_modulate")
# The fused encoder's contexts: launch flags, the queue's max_queue_cbs (0: 162), the caller's limit on a batch's staged
# bytes (None: none), the kinds of rows (None: all). csrc/ldpc_hip_enc_queue.cpp launch(): a batch that stages at most
# 1 MiB (messages and outputs) is zero-copy, unless LDPC_HIP_LAUNCH_HAL_COPY; a zero-copy batch of at most 8
# codeblocks goes to the device work queue (ldpc_dwq_encode_kernel), unless LDPC_HIP_LAUNCH_NO_DWQ; every other batch is
# one launch of ldpc_pdsch_encode_kernel, a single codeblock's descriptor by value.
ENC_CONTEXTS = {
    "work_queue_8": ((), 8, 1 << 20, None),
    "launch": (("LAUNCH_NO_DWQ",), 0, 1 << 20, None),
    "launch_copy": (("LAUNCH_NO_DWQ", "LAUNCH_HAL_COPY"), 0, None, None),
    "launch_by_value": (("LAUNCH_NO_DWQ",), 1, 1 << 20, ("staging", "division", "wrap")),
}


def route_skip(route, c):
    """The one place a device route may leave a row out: the reason, or None when the route takes the row. Today every
    route takes every row: the C ABI admits rm_length up to 2^31 - 1 on all three, CB mode takes any (bg, Z, E, Qm, rv,
    Nref, F), and BPSK goes to the fused modulator as modulation 1. tests/test_rm_grid.py asserts the count per
    route."""
    assert route in ROUTES
    return None
