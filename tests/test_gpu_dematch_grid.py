"""The rate dematcher's soft buffers at every allot branch, workgroup width and route: the grid of
tests/dematch_grid.py (19 branch rows on 12 graphs, 18 width rows on 4) through every device entry point that runs
dematch_body (csrc/ldpc_dematch_body.h), compared with the oracle (oracle/ldpc_oracle.c, held to the compiled reference
on the same grid by tests/test_oracle_vs_reference.py and tests/golden/ref_dematch_grid.json).

Per route all codeblocks go into one plan and one launch per transmission: (1) new data over a stale 'harq' buffer,
(2) a combine of the second transmission into that result, (3) a combine of the first transmission into a fresh copy
of the stale buffer. After each, every codeblock's whole soft buffer equals the oracle's and, in the fused forms, the
decoded message (2 iterations, no CRC) equals the oracle decoder's on the oracle's soft buffer: the decoder's prologue
saw the stores of its own workgroup's dematcher. Every comparison is exact integer equality.

Every second codeblock's soft buffer starts at an offset = 5 (mod 16) and its LLR input at = 3 (mod 16), the others at
= 0; 64 guard bytes of 99 lie between neighbouring soft buffers, outputs and LLR inputs and still hold 99 afterwards.

The symbol and scrambled forms leave out the rows with E > 32768 or E = 0 (tests/dematch_grid.fits_staging), by that
rule and no other: the host refuses to demodulate or descramble what the LDS staging cannot hold. The oracle's side is
computed once per module and shared by the routes. Each test prints its codeblock count and wall time."""
import ctypes
import time

import numpy as np
import pytest

import oracle as O
from tests import dematch_grid as G
from tests import ref_cases as C
from tests import scrambling_ref as R
from tests.vectors import sm_symbols

pytestmark = pytest.mark.gpu

ITERS = 2
GUARD = 64
TX = (("soft_new", 1, True), ("soft_comb", 2, False), ("soft_comb0", 1, False))  # result, which input, new_data
# c_init values of the descrambler fixture; sequence offsets that are no multiples of 32, one above 2^16
SEQS = [(c["c_init"], off) for c, off in zip(C.descramble_cases(), (7, 31, 1249, 70001, 3, 33, 515, 65))]
ROUTES = {"mixed": 0, "per_group": "LAUNCH_NO_MIXED", "generic": "LAUNCH_NO_SPEC",
          "narrow": "LAUNCH_NARROW_ALWAYS|LAUNCH_NO_MIXED|LAUNCH_NO_SPEC"}
_EXP = {}


def _N(c):
    return O.BG_N_SHORT[c["bg"]] * c["Z"]


def _scr_of(cases):
    """Per codeblock None or (c_init, seq_offset): every second codeblock that fits the LDS staging is scrambled."""
    out, k = [], 0
    for c in cases:
        if G.fits_staging(c):
            out.append(SEQS[(k // 2) % len(SEQS)] if k % 2 else None)
            k += 1
        else:
            out.append(None)
    return out


def _mod_of(cases):
    """modulation_scheme per codeblock: Qm, and the Qm = 1 rows alternate BPSK (1) and pi/2-BPSK (0)."""
    out, k = [], 0
    for c in cases:
        out.append(c["Qm"] if c["Qm"] > 1 else k % 2)
        k += c["Qm"] == 1
    return out


def _expected(form):
    """form 'llr': every grid case with tests/ref_cases.dematch_input's transmissions. form 'sym': the cases that fit
    the staging; the transmissions are the oracle demodulator's LLRs of seeded symbols, descrambled on every second
    codeblock. Returns cases, device inputs and, per case, the oracle's three soft buffers and decoded messages."""
    if form not in _EXP:
        cases = G.grid_cases() if form == "llr" else [c for c in G.grid_cases() if G.fits_staging(c)]
        scr, mods = _scr_of(cases), _mod_of(cases)
        inputs, dev, want = [], [], []
        for c, s, mod in zip(cases, scr, mods):
            start, tx1, tx2 = C.dematch_input(c)
            if form == "sym":
                syms = [sm_symbols(c["seed"] + 10 + k, c["E"] // c["Qm"], mod) for k in (0, 1)]
                tx1, tx2 = [O.demodulate_soft(mod, *sv) for sv in syms]
                if s is not None:
                    tx1, tx2 = R.descramble(tx1, *s), R.descramble(tx2, *s)
                dev.append(syms)
            inp = (start, tx1, tx2)
            soft = C.run_dematch(C.ORACLE, c, inp)
            msg = {k: O.ldpc_decode(c["bg"], c["Z"], v, ITERS, O.NO_CRC, c["F"])[0] for k, v in soft.items()}
            for a in list(soft.values()) + list(msg.values()) + list(inp):
                a.setflags(write=False)
            inputs.append(inp)
            want.append((soft, msg))
        _EXP[form] = dict(cases=cases, scr=scr, mods=mods, inputs=inputs, dev=dev, want=want)
    return _EXP[form]


def test_grid_counts():
    """What the launches below compare: 300 codeblocks, 285 in the symbol and scrambled forms."""
    cases = G.grid_cases()
    assert len(cases) == 300 and sum(G.fits_staging(c) for c in cases) == 300 - 12 - 3
    assert sum(s is not None for s in _scr_of(cases)) == 142
    assert any(off > 1 << 16 for _, off in SEQS) and all(off % 32 for _, off in SEQS)


def _layout(sizes, odd_shift):
    """Offsets of arrays of `sizes` in one buffer: array k starts at a multiple of 16 (+ odd_shift for odd k), GUARD
    bytes or more lie before, between and after them. Returns (offsets, total)."""
    offs, pos = [], GUARD
    for k, n in enumerate(sizes):
        pos = (pos + 15) // 16 * 16 + (odd_shift if k % 2 else 0)
        offs.append(pos)
        pos += n + GUARD
    return offs, (pos + 15) // 16 * 16


def _fill(offs, arrays, total, dtype=np.int8):
    h = np.full(total, 99, dtype)
    for o, a in zip(offs, arrays):
        h[o:o + a.size] = a
    return h


def _guards_hold(what, got, offs, sizes):
    mask = np.ones(got.size, bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
    bad = np.flatnonzero(mask & (got != 99))
    assert bad.size == 0, f"{what}: {bad.size} guard bytes changed, first at {bad[:4]} (buffers start at {offs[:4]}...)"


def _same(what, cases, got, offs, want):
    bad = []
    for c, o, w in zip(cases, offs, want):
        g = got[o:o + w.size]
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            bad.append(f"BG{c['bg']} Z={c['Z']} {c['row']} (Qm {c['Qm']} rv {c['rv']} F {c['F']} Nref {c['Nref']} "
                       f"E {c['E']}): {int((g != w).sum())} differ, first at {i}: {g[i]} != {w[i]}")
    assert not bad, f"{what}: {len(bad)} of {len(cases)} codeblocks differ:\n" + "\n".join(bad[:12])


def _dm_descs(cases, new_data):
    from srsran_projectvtlmo_amd import _lib
    dm = (_lib.DematchDesc * len(cases))()
    for d, c in zip(dm, cases):
        d.modulation_order, d.rv, d.new_data = c["Qm"], c["rv"], int(new_data)
        d.cb_length, d.rm_length, d.Nref, d.nof_filler_bits = _N(c), c["E"], c["Nref"], c["F"]
    return dm


class _Inputs:
    """One transmission's device input of every codeblock: LLRs (scrambled where scr says so) or symbols."""

    def __init__(self, e, which, symbols, scr):
        import torch
        from srsran_projectvtlmo_amd import channel_modulation as cm
        from srsran_projectvtlmo_amd import sequence_generators as sg
        n = len(e["cases"])
        self.scr = sg.scramble_descriptors(scr) if scr is not None else None
        self.demod = self.d_sym = self.d_nv = self.d_llr = self.offs = None
        if symbols:
            syms = [d[which - 1] for d in e["dev"]]
            so = np.cumsum([0] + [s[0].size for s in syms])
            self.demod = cm.demod_descriptors([cm.demod_segment(s[0].size, m, int(o), int(o), 0)
                                               for s, m, o in zip(syms, e["mods"], so)])
            self.d_sym = torch.from_numpy(np.concatenate([s[0] for s in syms]).view(np.float32)).cuda()
            self.d_nv = torch.from_numpy(np.concatenate([s[1] for s in syms])).cuda()
        else:
            txs = [i[which] if s is None else R.descramble(i[which], *s)
                   for i, s in zip(e["inputs"], scr if scr is not None else [None] * n)]
            self.sizes = [t.size for t in txs]
            offs, total = _layout(self.sizes, 3)
            self.host = _fill(offs, txs, total)
            self.d_llr = torch.from_numpy(self.host).cuda()
            self.offs = (ctypes.c_uint64 * n)(*offs)
            self.off_list = offs

    def ptr(self, t):
        return t.data_ptr() if t is not None else None

    def check_guards(self, what):
        if self.d_llr is not None:
            got = self.d_llr.cpu().numpy()
            assert np.array_equal(got, self.host), f"{what}: the LLR input changed"
            _guards_hold(what + " LLR input", got, self.off_list, self.sizes)


def _run(ctx, form, what, fused, scr_llr=False):
    """The three transmissions of every codeblock of the form through one launch each. fused: a decode plan and
    ldpc_hip_dematch_decode(_scr)_launch; else ldpc_hip_rate_dematch_scr_launch. Returns the codeblock count."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    e = _expected(form)
    cases, n = e["cases"], len(e["cases"])
    symbols = form == "sym"
    scr = e["scr"] if (symbols or scr_llr) else None
    assert n == (285 if symbols else 300)
    sizes = [_N(c) for c in cases]
    soft_off, soft_total = _layout(sizes, 5)
    assert {o % 16 for o in soft_off} == {0, 5}
    msg_sizes = [cc.message_bytes(c["bg"], c["Z"]) for c in cases]
    out_off, out_total = _layout(msg_sizes, 0)
    stale = _fill(soft_off, [i[0] for i in e["inputs"]], soft_total)
    d_soft = torch.from_numpy(stale).cuda()
    d_out = torch.full((out_total,), 99, dtype=torch.uint8, device="cuda")
    plan = None
    if fused:
        plan = cc.DecodePlan(ctx, [cc.cb_decode_spec(c["bg"], c["Z"], _N(c), ITERS, cc.CRC_MODE_NONE, 0, c["F"], 0.8,
                                                     so, oo) for c, so, oo in zip(cases, soft_off, out_off)])
    u64 = ctypes.c_uint64 * n
    try:
        for name, which, new_data in TX:
            if name == "soft_comb0":
                d_soft.copy_(torch.from_numpy(stale))
            d_out.fill_(99)
            inp = _Inputs(e, which, symbols, scr)
            dm = _dm_descs(cases, new_data)
            if fused:
                rc = ctx.lib.ldpc_hip_dematch_decode_scr_launch(
                    plan.handle, dm, inp.ptr(inp.d_llr), inp.offs, inp.demod, inp.ptr(inp.d_sym), inp.ptr(inp.d_nv),
                    inp.scr, d_soft.data_ptr(), d_out.data_ptr(), None, _lib.stream_arg(0))
            else:
                rc = ctx.lib.ldpc_hip_rate_dematch_scr_launch(
                    ctx.handle, n, dm, inp.ptr(inp.d_llr), inp.offs, inp.demod, inp.ptr(inp.d_sym), inp.ptr(inp.d_nv),
                    inp.scr, d_soft.data_ptr(), u64(*soft_off), _lib.stream_arg(0))
            assert rc == 0, ctx.lib.ldpc_hip_last_error(ctx.handle).decode()
            torch.cuda.synchronize()
            soft = d_soft.cpu().numpy()
            _same(f"{what} {name} soft buffer", cases, soft, soft_off, [w[0][name] for w in e["want"]])
            _guards_hold(f"{what} {name} soft", soft, soft_off, sizes)
            inp.check_guards(f"{what} {name}")
            out = d_out.cpu().numpy()
            if fused:
                _same(f"{what} {name} decoded message", cases, out, out_off, [w[1][name] for w in e["want"]])
                _guards_hold(f"{what} {name} output", out, out_off, msg_sizes)
            else:
                assert np.all(out == 99)
    finally:
        if plan is not None:
            plan.close()
    return n


def _route_ctx(hip_ctx, route):
    from srsran_projectvtlmo_amd import _lib
    flags = ROUTES[route]
    if flags == 0:
        return hip_ctx, False
    bits = 0
    for name in flags.split("|"):
        bits |= getattr(_lib, name)
    return _lib.Context(0, max_queue_cbs=256, nof_harq_slots=0, launch_flags=bits), True


def _timed(what, hip_ctx, route, fn):
    ctx, own = _route_ctx(hip_ctx, route)
    _expected("llr"), _expected("sym")  # the oracle's side, once per module, outside the timing
    t0 = time.perf_counter()
    try:
        n = fn(ctx)
    finally:
        if own:
            ctx.close()
    print(f"{what}[{route}]: {n} codeblocks x 3 transmissions compared, {time.perf_counter() - t0:.2f} s")
    return n


@pytest.mark.parametrize("route", list(ROUTES))
def test_fused_llr_input(hip_ctx, route):
    """ldpc_hip_dematch_decode_launch on the mixed launch, each specialised body's own launch, the generic body and
    the narrow schedule: every branch and width row. The rows with E > 32768 make the launch mix staged and unstaged
    codeblocks under one stage_bytes budget (dm_fused_budget)."""
    e = _expected("llr")
    assert any(c["E"] > C.DM_STAGE for c in e["cases"]) and any(c["E"] == 0 for c in e["cases"])
    assert _timed("fused, LLR input", hip_ctx, route, lambda ctx: _run(ctx, "llr", f"fused LLR [{route}]", True)) == 300


@pytest.mark.parametrize("route", list(ROUTES))
def test_fused_symbol_input(hip_ctx, route):
    """ldpc_hip_dematch_decode_scr_launch with demod != NULL on the same four routes: the expected LLRs are the oracle
    demodulator's, the Qm = 1 rows alternate BPSK and pi/2-BPSK, every second codeblock is scrambled."""
    e = _expected("sym")
    assert {0, 1, 2, 4, 6, 8} == set(e["mods"]) and sum(s is not None for s in e["scr"]) == 142
    assert _timed("fused, symbol input", hip_ctx, route,
                  lambda ctx: _run(ctx, "sym", f"fused symbols [{route}]", True)) == 285


@pytest.mark.parametrize("route", ["mixed", "per_group"])
def test_fused_scrambled_llr_input(hip_ctx, route):
    """LLR input, every second staged codeblock scrambled (the descrambler's equal runs over the decoder's width),
    the unstaged and the empty ones in the same launch."""
    assert _timed("fused, scrambled LLR input", hip_ctx, route,
                  lambda ctx: _run(ctx, "llr", f"fused scrambled LLR [{route}]", True, scr_llr=True)) == 300


@pytest.mark.parametrize("form", ["llr", "scrambled_llr", "symbols"])
def test_standalone_kernel(hip_ctx, form):
    """The 512-thread kernel (ldpc_hip_rate_dematch_scr_launch) on the whole grid in its three input forms."""
    n = _timed(f"stand-alone kernel, {form}", hip_ctx, "mixed",
               lambda ctx: _run(ctx, "sym" if form == "symbols" else "llr", f"stand-alone {form}", False,
                                scr_llr=form == "scrambled_llr"))
    assert n == (285 if form == "symbols" else 300)


@pytest.mark.parametrize("dwq", [True, False], ids=["work_queue", "no_work_queue"])
def test_one_cb_sync(hip_ctx, dwq):
    """ldpc_rate_dematcher_hip (the one-codeblock sync call: a work-queue item, or a one-block launch with
    LAUNCH_NO_DWQ) on the branch rows of (2,3), (1,36) and (1,384); host buffers, every second one 5 bytes off a
    16-byte boundary of its array, 64 guard bytes of 99 around each."""
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    e = _expected("llr")
    pick = [k for k, c in enumerate(e["cases"])
            if c["kind"] == "branch" and (c["bg"], c["Z"]) in ((2, 3), (1, 36), (1, 384))]
    assert len(pick) == 57
    ctx = hip_ctx if dwq else _lib.Context(0, max_queue_cbs=256, nof_harq_slots=0, launch_flags=_lib.LAUNCH_NO_DWQ)
    t0 = time.perf_counter()
    try:
        dm = cc.ldpc_rate_dematcher_hip(ctx)
        bad = []
        for j, k in enumerate(pick):
            c, (start, tx1, tx2), (want, _) = e["cases"][k], e["inputs"][k], e["want"][k]
            meta = cc.codeblock_metadata()
            meta.tb_common.rv, meta.tb_common.mod, meta.tb_common.Nref = c["rv"], c["Qm"], c["Nref"]
            meta.cb_specific.nof_filler_bits = c["F"]
            N, sh = start.size, GUARD + (5 if j % 2 else 0)
            bufs = [np.full(N + 2 * GUARD + 16, 99, np.int8) for _ in range(2)]
            a, b = bufs[0][sh:sh + N], bufs[1][sh:sh + N]
            a[:], b[:] = start, start
            dm.rate_dematch(a, tx1, True, meta)
            got = {"soft_new": a.copy()}
            dm.rate_dematch(a, tx2, False, meta)
            dm.rate_dematch(b, tx1, False, meta)
            got.update(soft_comb=a, soft_comb0=b)
            names = C.compare(got, want)
            if names:
                bad.append(f"BG{c['bg']} Z={c['Z']} {c['row']}: {names}")
            for buf in bufs:
                assert np.all(buf[:sh] == 99) and np.all(buf[sh + N:] == 99), f"guard bytes changed: {c}"
        assert not bad, f"{len(bad)} of {len(pick)} codeblocks differ:\n" + "\n".join(bad[:12])
    finally:
        if not dwq:
            ctx.close()
    print(f"one-codeblock sync[{'work queue' if dwq else 'no work queue'}]: {len(pick)} codeblocks x 3 transmissions "
          f"compared, {time.perf_counter() - t0:.2f} s")
