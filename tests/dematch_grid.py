"""The rate dematcher's branch grid: cases that reach every branch of the allot loop
(ldpc_rate_dematcher_impl.cpp:128-201, csrc/ldpc_dematch_body.h) on graphs of every decoder body, and E / Qm around
every workgroup width the fused dematcher runs at. tests/test_dematch_grid.py checks the grid's own conditions on the
CPU, tests/ref_cases.live_dematch_cases() and tests/golden/ref_dematch_grid.json hold the oracle to the reference on it,
and tests/test_gpu_dematch_grid.py holds every device entry point to the oracle on it.

A case is tests/ref_cases.dematch_case's dict of plain numbers plus the name of its row; its inputs are
tests/ref_cases.dematch_input's ('harq' LLRs for the stale buffer and both transmissions).

allot_trace() restates the loop's control flow only (it moves no data) and names what a case reaches:

  start        k0_info, k0_filler (ninfo < k0 < nsys), k0_eq_ninfo, k0_parity   (of a case with E > 0)
  systematic   sys_copy, sys_comb, sys_skip_copy (copy mode with tmp_idx >= ninfo: zero_fill(0, ninfo)), sys_skip_comb,
               zero_head (copy mode from tmp_idx > 0: the systematic part below it is zeroed), fill (F > 0, copy mode)
  end          end_in_info, end_at_ninfo, end_in_parity, end_at_ncb (= wrap_exact)
  parity       par0 (empty range), par1 (one element), par_copy, par_comb
  wrap         wrap (the transmission goes on at the start of the buffer), wrap_exact (its last LLR lands on Ncb - 1)
  passes       passes0 (E = 0), passes1, passes2, passes3 (three or more)
  tail         tail_zero, tail_zero_lbrm (Ncb < N: the LAST Ncb - tmp_idx entries of the N-sized buffer), no_tail

Workgroup widths (threads) the dematcher runs at, read from csrc/ldpc_spec.h (make_spec, make_quad),
csrc/ldpc_graph.cpp (build_tasks) and csrc/ldpc_hip_device.h (MIXED_BLOCK, DM_THREADS):

  route                              width
  stand-alone kernel, sync call      512 (DM_THREADS)
  mixed launch (default context)     768 (MIXED_BLOCK) for every codeblock of the launch, whatever its graph
  specialised body's own launch      lane-split graphs (Z <= 64): 64 * 2 * ceil(P Z / 64), P = 4 up to Z = 32, else 2:
  (LAUNCH_NO_MIXED)                    (1,2) (2,3) (1,7) (2,15) 128; (1,36) (2,36) (2,64) 256
                                     others: 64 * max(2 ceil(Z / 64), ceil(Z / 32)):
                                       (1,104) 256; (2,208) 512; (1,256) 512; (2,384) (1,384) 768
  generic body (LAUNCH_NO_SPEC)      64 * max(4, chunks of the widest step), at most 1024: 256 on the small graphs, up
                                     to 1024 on the large ones (a step's chunks: its rows x ceil(Z / 64), or / 32 split)
  narrow schedule                    the generic body with steps of at most 8 waves: 256 to 512

The table is documentation: no test depends on it. The width rows put E / Qm just below, at and above 64 .. 1024, so
whatever width a route picks, dq = nth div EQ and dr = nth mod EQ take the values 0, >= 1 and 0, != 0 among them."""
from __future__ import annotations

import oracle as O
from tests.ref_cases import DM_STAGE, dematch_case

BRANCH_GRAPHS = [(1, 2), (2, 3), (1, 7), (2, 15), (1, 36), (2, 36), (2, 64), (1, 104), (2, 208), (1, 256), (2, 384),
                 (1, 384)]
WIDTH_GRAPHS = [(2, 3), (1, 36), (2, 208), (1, 384)]
WIDTH_EQ = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
QMS = (1, 2, 4, 6, 8)
MAX_CODEBLOCK_RM_SIZE = 384 * 22 * 35  # the reference's ldpc.h: MAX_MESSAGE_SIZE * 35
SF = {1: (0, 17, 33, 56), 2: (0, 13, 25, 43)}

LABELS = frozenset("""k0_info k0_filler k0_eq_ninfo k0_parity sys_copy sys_comb sys_skip_copy end_in_info end_at_ninfo
par0 par1 par_copy par_comb wrap wrap_exact passes0 passes1 passes2 passes3 tail_zero tail_zero_lbrm no_tail""".split())
EXTRA_LABELS = frozenset("sys_skip_comb zero_head fill end_in_parity end_at_ncb".split())


def geometry(bg, Z, rv=0, F=0, Nref=0):
    """N, nsys, ninfo, Ncb, k0, lap of a codeblock, as the reference computes them (:53-105)."""
    N, nsys = O.BG_N_SHORT[bg] * Z, (O.BG_K[bg] - 2) * Z
    Ncb = min(Nref, N) if Nref > 0 else N
    k0 = (SF[bg][rv] * Ncb) // N * Z
    return dict(N=N, nsys=nsys, ninfo=nsys - F, Ncb=Ncb, k0=k0, lap=Ncb - F)


def allot_trace(bg, Z, E, rv, Qm, F, Nref, new_data) -> set:
    """The labels (module docstring) the allot loop reaches for this case. Qm does not steer the loop."""
    g = geometry(bg, Z, rv, F, Nref)
    N, nsys, ninfo, Ncb, k0 = g["N"], g["nsys"], g["ninfo"], g["Ncb"], g["k0"]
    assert E % Qm == 0 and F < nsys and Ncb >= nsys
    got = set()
    if E > 0:
        got.add("k0_info" if k0 < ninfo else "k0_eq_ninfo" if k0 == ninfo else "k0_filler" if k0 < nsys
                else "k0_parity")
    copy, tmp, left, passes = bool(new_data), k0, E, 0
    while left != 0:
        passes += 1
        if tmp < ninfo:
            n = min(ninfo - tmp, left)
            got.add("sys_copy" if copy else "sys_comb")
            if copy and tmp > 0:
                got.add("zero_head")
            tmp += n
            left -= n
            if left == 0:
                got.add("end_at_ninfo" if tmp == ninfo else "end_in_info")
        else:
            got.add("sys_skip_copy" if copy else "sys_skip_comb")
        if copy and F > 0:
            got.add("fill")
        tmp = max(tmp, nsys)
        had = left
        np_ = min(Ncb - tmp, left)
        got.add("par0" if np_ == 0 else "par1" if np_ == 1 else "par_copy" if copy else "par_comb")
        if np_ == 1:
            got.add("par_copy" if copy else "par_comb")
        left -= np_
        if had and left == 0 and tmp + np_ < Ncb:
            got.add("end_in_parity")
        if tmp + np_ == Ncb and had:
            got.update(("wrap",) if left else ("wrap_exact", "end_at_ncb"))
        tmp = (tmp + np_) % Ncb
        if left:
            copy = False
    got.add(f"passes{min(passes, 3)}")
    if copy and tmp != 0:
        got.add("tail_zero" if Ncb == N else "tail_zero_lbrm")
    else:
        got.add("no_tail")
    return got


def up(E, Qm):
    return (E + Qm - 1) // Qm * Qm


def qm_dividing(E, Qm):
    """Qm, or the next smaller modulation order that divides E (for rows whose length is meant exactly)."""
    return next(q for q in reversed(QMS) if q <= Qm and E % q == 0)


def branch_rows(bg, Z):
    """19 (name, Qm, rv, F, Nref, E) rows built from the graph's own ninfo, nsys, Ncb, k0 and lap = Ncb - F. E is
    rounded up to a multiple of Qm, except in the rows named 'exact', which take the largest modulation order up to the row's
    that divides the length they are about. On BG2 rv 1 starts in the parity part of an unlimited buffer, so its two
    filler rows limit the buffer to nsys + 1 (k0 = 2 Z)."""
    N, nsys = O.BG_N_SHORT[bg] * Z, (O.BG_K[bg] - 2) * Z
    Fh, mid = Z // 2 + 1, (nsys + N) // 2 + 3
    fill_nref = 0 if bg == 1 else nsys + 1

    def g(rv=0, F=0, Nref=0):
        return geometry(bg, Z, rv, F, Nref)

    k0f = g(1, 0, fill_nref)["k0"]  # k0 does not depend on F
    assert 0 < nsys - k0f + 5 < nsys
    rows = [
        ("end_in_info", 1, 0, 0, 0, nsys - 1, False),
        ("end_at_ninfo_exact", 2, 0, Fh, 0, nsys - Fh, True),
        ("one_lap_exact", 4, 0, 0, 0, g()["lap"], True),
        ("one_lap_plus_1_exact", 6, 0, Fh, 0, g(0, Fh)["lap"] + 1, True),
        ("multi_lap", 8, 0, 0, 0, 2 * N + N // 3, False),
        ("rv1_short", 2, 1, 0, 0, Z + 3, False),
        ("k0_in_fillers", 4, 1, nsys - k0f + 5, fill_nref, Z + 3, False),
        ("k0_at_ninfo_exact", 6, 1, nsys - k0f, fill_nref, g(1, nsys - k0f, fill_nref)["lap"] + 1, True),
        ("rv2_fillers_short", 8, 2, Fh, 0, Z + 3, False),
        ("rv2_to_end_exact", 1, 2, 0, 0, N - g(2)["k0"], True),
        ("rv3_to_end_plus_1_exact", 2, 3, 0, 0, N - g(3)["k0"] + 1, True),
        ("lbrm_min_rv3", 4, 3, Fh, nsys + 1, Z + 3, False),
        ("lbrm_min_multi_lap", 6, 2, 0, nsys + 1, 2 * (nsys + 1) + (nsys + 1) // 3, False),
        ("lbrm_n_minus_1_lap", 8, 3, 0, N - 1, N - 1, False),
        ("lbrm_mid_to_end_plus_1_exact", 1, 3, Fh, mid, mid - g(3, Fh, mid)["k0"] + 1, True),
        ("lbrm_mid_at_ninfo_exact", 2, 0, 0, mid, nsys, True),
        # Nref above N, up to the largest value the reference and the host accept (MAX_CODEBLOCK_SIZE)
        ("nref_above_n_one_llr", 1, 1, 0, min(N + 5, 66 * 384), 1, True),
        ("lbrm_mid_one_symbol", 8, 1, 0, mid, 8, True),
        ("empty", 2, 2, 0, 0, 0, True),
    ]
    out = []
    for name, Qm, rv, F, Nref, E, exact in rows:
        if exact:
            Qm = qm_dividing(E, Qm)
        out.append((name, Qm, rv, F, Nref, up(E, Qm)))
    return out


def width_rows(bg, Z):
    """rv 0, F 0, E = EQ * Qm with EQ just below, at and above every workgroup width; on a small graph many laps."""
    return [(f"width_{eq}", QMS[i % 5], 0, 0, 0, eq * QMS[i % 5]) for i, eq in enumerate(WIDTH_EQ)]


def grid_cases():
    """Every case of the grid, in a fixed order: the branch rows of BRANCH_GRAPHS, then the width rows of WIDTH_GRAPHS.
    Seeds 24000 + 3 i (the dematch input takes seed, seed + 1, seed + 2)."""
    cases = []
    for kind, graphs, rows in (("branch", BRANCH_GRAPHS, branch_rows), ("width", WIDTH_GRAPHS, width_rows)):
        for bg, Z in graphs:
            for name, Qm, rv, F, Nref, E in rows(bg, Z):
                c = dematch_case(bg, Z, E, rv, Qm, F, Nref, 24000 + 3 * len(cases))
                c["row"], c["kind"] = name, kind
                cases.append(c)
    return cases


def trace_of(c, new_data):
    return allot_trace(c["bg"], c["Z"], c["E"], c["rv"], c["Qm"], c["F"], c["Nref"], new_data)


def labels_of(c):
    """What the case's three transmissions reach together (new data; combine)."""
    return trace_of(c, True) | trace_of(c, False)


def fits_staging(c):
    """The one rule of the symbol and scrambled forms: the dematcher demodulates / descrambles in its LDS staging, which
    holds DM_STAGE LLRs, and a symbol descriptor needs at least one symbol."""
    return 0 < c["E"] <= DM_STAGE

