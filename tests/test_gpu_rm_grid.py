"""The three device rate matchers at every branch of the bit selection, on every lifted graph and around every staging
boundary: the rows of tests/rm_grid.py (20 branch rows on 12 graphs, one row on each of the 102 graphs, 66 staging
rows) through

  1. rate_match_launch               ldpc_rate_match_kernel: a packed codeword in HBM, a remainder per bit
  2. hal.hw_accelerator_pdsch_enc    ldpc_dwq_encode_kernel / ldpc_pdsch_encode_kernel: enc_build and pdsch_rate_match
     (CB mode, tests/pdsch_flow.        in one workgroup, the codeword's columns in LDS, a float-reciprocal division
     encode_cbs)                        below r0 + E = 2^21 and an exact one above, 4096 output bytes staged per chunk;
                                        batches kept at or below the 1 MiB up to which the queue stays zero-copy,
                                        except in the copy context
  3. rate_match_modulate_launch      mod_rate_match: one remainder per (chunk, bit of the symbol), then a step with a
                                      wrap test per symbol; a thread's chunk holds 32, 16, 8, 16, 4 symbols for
                                      Qm = 1, 2, 4, 6, 8 (mod_chunk_syms in csrc/ldpc_modulation_kernels.hip)

compared with the oracle (oracle/ldpc_oracle.c orc_ldpc_encode + orc_rate_match, held to the compiled reference on the
same rows by tests/test_oracle_vs_reference.py and tests/golden/ref_rate_match_grid.json). Every comparison is exact
equality of bits (route 3: of the ci8 levels tests/modulation_ref.py gives for the oracle's bits, scrambled by
tests/scrambling_ref.py or not). tests/rm_grid.route_skip is the one place a route may leave a row out; it leaves none
out (tests/test_rm_grid.py asserts the counts). The oracle's side is computed once per module and shared by the routes.
Each test prints its codeblock count and wall time."""
import functools
import time

import numpy as np
import pytest

import oracle as O
from tests import modulation_ref as M
from tests import ref_cases as C
from tests import rm_grid as G
from tests import scrambling_ref as R
from tests.pdsch_flow import ENC_ZERO_COPY_MAX_BYTES, cb_staged_bytes, encode_cbs, plan_batches

pytestmark = pytest.mark.gpu
FILL = 0xEE


def _N(c):
    return O.BG_N_SHORT[c["bg"]] * c["Z"]


def _up16(n):
    return (n + 15) // 16 * 16


@functools.lru_cache(maxsize=1)
def _data():
    """Per row: the message, the oracle's codeword and rate-matched bits (read-only)."""
    rows = G.all_rows()
    msgs = [C.rm_message(c) for c in rows]
    cws = [O.ldpc_encode(c["bg"], c["Z"], m) for c, m in zip(rows, msgs)]
    bits = [O.rate_match(cw, c["E"], c["rv"], c["Qm"], c["Nref"], c["bg"], c["Z"]) for c, cw in zip(rows, cws)]
    for a in msgs + cws + bits:
        a.setflags(write=False)
    return rows, msgs, cws, bits


def _kept(route, only=None):
    rows, msgs, cws, bits = _data()
    idx = [i for i, c in enumerate(rows) if G.route_skip(route, c) is None and (only is None or c["kind"] in only)]
    return [rows[i] for i in idx], [msgs[i] for i in idx], [cws[i] for i in idx], [bits[i] for i in idx]


def _packed_cw(cw):
    return np.packbits(np.where(cw == O.FILLER_BIT, 0, cw).astype(np.uint8))


def _describe(c):
    return {k: c[k] for k in ("bg", "Z", "E", "rv", "Qm", "F", "Nref", "row")}


def _rate_match_on_device(hip_ctx, rows, cws):
    """rate_match_launch of the rows in one launch, output offsets at 16-byte steps over a buffer of FILL bytes.
    Returns (the buffer, the offsets)."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    specs, coffs, ooffs = [], [], []
    co = oo = 0
    for c in rows:
        specs.append(cc.cb_rate_match_spec(_N(c), c["E"], c["Qm"], c["rv"], c["Nref"], c["F"], co, oo))
        coffs.append(co)
        ooffs.append(oo)
        co += _up16((_N(c) + 7) // 8)
        oo += _up16((c["E"] + 7) // 8)
    h = np.zeros(co, np.uint8)
    for off, cw in zip(coffs, cws):
        p = _packed_cw(cw)
        h[off:off + p.size] = p
    d_cw = torch.from_numpy(h).cuda()
    d_out = torch.full((oo,), FILL, dtype=torch.uint8, device="cuda")
    cc.rate_match_launch(hip_ctx, specs, d_cw.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), ooffs


def test_rate_match_launch(hip_ctx):
    """Route 1. Every row's packed bytes (the last byte's unused bits zero) and the FILL bytes up to the next row."""
    t0 = time.time()
    rows, _, cws, bits = _kept("rate_match_launch")
    got, offs = _rate_match_on_device(hip_ctx, rows, cws)
    bad = []
    for c, off, want in zip(rows, offs, bits):
        nb = (c["E"] + 7) // 8
        pad = got[off + nb:off + _up16(nb)]
        if not np.array_equal(got[off:off + nb], np.packbits(want)) or not np.all(pad == FILL):
            bad.append(_describe(c))
    print(f"rate_match_launch: {len(rows)} codeblocks, {time.time() - t0:.1f} s")
    assert len(rows) == 408 and not bad, f"{len(bad)} of {len(rows)} rows differ from the oracle, first: {bad[:5]}"


def _which_half(c, msg, cw, want):
    """For a row the fused encoder got wrong: does encode_launch of the same message give the oracle's codeword, and
    does rate_match_launch of the oracle's codeword give the oracle's bits? (A context of its own.)"""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    ctx = _lib.Context(0)
    try:
        N = _N(c)
        d_msg = torch.from_numpy(np.concatenate([_packed_cw(msg), np.zeros(16, np.uint8)])).cuda()
        d_cw = torch.zeros(_up16((N + 7) // 8), dtype=torch.uint8, device="cuda")
        cc.encode_launch(ctx, [cc.cb_encode_spec(c["bg"], c["Z"], N, 0, 0)], d_msg.data_ptr(), d_cw.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        enc_ok = np.array_equal(d_cw.cpu().numpy()[:(N + 7) // 8], _packed_cw(cw))
        got, _ = _rate_match_on_device(ctx, [c], [cw])
        rm_ok = np.array_equal(got[:(c["E"] + 7) // 8], np.packbits(want))
    finally:
        ctx.close()
    return (f"encode_launch of its message {'equals' if enc_ok else 'DIFFERS from'} O.ldpc_encode, rate_match_launch "
            f"of the oracle's codeword {'equals' if rm_ok else 'DIFFERS from'} O.rate_match")


@pytest.mark.parametrize("name", list(G.ENC_CONTEXTS))
def test_fused_encoder(name):
    """Route 2, CB mode, in the four contexts of tests/rm_grid.ENC_CONTEXTS. The queue takes a batch off its zero-copy
    routes (work queue, zero-copy launch) once the batch stages more than 1 MiB, and has no counter that tells which
    route a batch took; so in the zero-copy contexts encode_cbs closes a batch before that limit, and the batches it
    made are asserted to be the planned ones, each within the limit (and within 8 codeblocks for the work queue):
    by ldpc_hip_enc_queue::launch()'s own conditions every one of them, the batches holding the 'division' rows
    included, is eligible for the route the context is about. Both outputs of dequeue_operation: one bit per byte,
    and packed."""
    from srsran_projectvtlmo_amd import _lib, hal
    t0 = time.time()
    flags, max_cbs, max_bytes, kinds = G.ENC_CONTEXTS[name]
    rows, msgs, cws, bits = _kept("pdsch_encode", kinds)
    ctx = _lib.Context(0, launch_flags=sum(getattr(_lib, f) for f in flags))
    try:
        enc = hal.hw_accelerator_pdsch_enc_hip(ctx, cb_mode=True, max_queue_cbs=max_cbs)
        try:
            got, stats = encode_cbs(enc, rows, msgs, max_bytes)
        finally:
            enc.close()
    finally:
        ctx.close()
    bad = [i for i, ((block, packed), want) in enumerate(zip(got, bits))
           if not np.array_equal(block, want) or not np.array_equal(packed, np.packbits(want))]
    print(f"fused encoder, {name}: {len(rows)} codeblocks in {len(stats['batches'])} batches, largest "
          f"{max(n for _, _, n in stats['batches'])} bytes, {time.time() - t0:.1f} s")
    why = _which_half(rows[bad[0]], msgs[bad[0]], cws[bad[0]], bits[bad[0]]) if bad else ""
    assert not bad, (f"{len(bad)} of {len(rows)} rows differ from the oracle, first: "
                     f"{[_describe(rows[i]) for i in bad[:5]]}; of the first, {why}")
    assert len(rows) == (408 if kinds is None else 66)
    assert [(a, b) for a, b, _ in stats["batches"]] == plan_batches(rows, max_cbs, max_bytes)
    for a, b, n in stats["batches"]:
        assert n == sum(cb_staged_bytes(c) for c in rows[a:b]) and b - a <= (max_cbs or 162)
        assert max_bytes is None or n <= ENC_ZERO_COPY_MAX_BYTES


@pytest.mark.parametrize("scramble", [False, True], ids=["plain", "scrambled"])
def test_rate_match_modulate_launch(hip_ctx, scramble):
    """Route 3 in the ci8 format, without scrambling (x1 == 0) and with it (c_init per row, sequence from 0): the levels
    of tests/modulation_ref.py for the oracle's bits. BPSK rows go as modulation 1. Symbol offsets at multiples of 8
    over a buffer of sentinel elements, which stay untouched between the rows."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    t0 = time.time()
    rows, _, cws, bits = _kept("rate_match_modulate")
    rm, mods, coffs, soffs = [], [], [], []
    co, so = 0, 8
    for k, c in enumerate(rows):
        n = c["E"] // c["Qm"]
        rm.append(cc.cb_rate_match_spec(_N(c), c["E"], c["Qm"], c["rv"], c["Nref"], c["F"], co, 0))
        mods.append(cm.mod_segment(n, c["Qm"], 0, so, scramble, (0x091A0155 + 7919 * k) & 0x7FFFFFFF if scramble else 0,
                                   0))
        coffs.append(co)
        soffs.append(so)
        co += _up16((_N(c) + 7) // 8)
        so += (n + 7) // 8 * 8 + 8
    h = np.zeros(co, np.uint8)
    for off, cw in zip(coffs, cws):
        p = _packed_cw(cw)
        h[off:off + p.size] = p
    d_cw = torch.from_numpy(h).cuda()
    d_sym = torch.full((so + 8, 2), 85, dtype=torch.int8, device="cuda")   # no level is 85
    cm.rate_match_modulate_launch(hip_ctx, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), _lib.SYM_CI8,
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_sym.cpu().numpy()
    bad, end = [], 0
    for c, m, s, want in zip(rows, mods, soffs, bits):
        b = want ^ R.sequence(m.c_init, 0, want.size) if scramble else want
        n = c["E"] // c["Qm"]
        if not np.array_equal(got[s:s + n], M.levels(b, c["Qm"])) or not np.all(got[end:s] == 85):
            bad.append(_describe(c))
        end = s + n
    print(f"rate_match_modulate_launch, {'scrambled' if scramble else 'plain'}: {len(rows)} codeblocks, "
          f"{time.time() - t0:.1f} s")
    assert np.all(got[end:] == 85)
    assert len(rows) == 408 and not bad, f"{len(bad)} of {len(rows)} rows differ from the oracle, first: {bad[:5]}"
