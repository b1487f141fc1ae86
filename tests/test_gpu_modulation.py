"""GPU tests of the modulation mapper (modulation_mapper_lut_impl.cpp on the device) and of the PDSCH scrambler in
front of it: the stand-alone mapper (ldpc_hip_modulate_sync / _launch) and rate matching fused with scrambling and
mapping (ldpc_hip_rate_match_modulate_launch). Expected values come from tests/modulation_ref.py (the integer nested
forms and the six float32 scalings) on bits scrambled by tests/scrambling_ref.py, and by the compiled reference where it
was built; every comparison is on bit patterns."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
from oracle import ref as REF
from tests import modulation_ref as M
from tests import scrambling_ref as R
from tests.tb_chain import TransportBlock

pytestmark = pytest.mark.gpu
C_INIT = 0x091A0155  # rnti 0x1234, q 0, n_id 0x155
FORMATS = ("cf32", "ci8")
SENTINEL = {"cf32": np.float32(12345.0), "ci8": np.int8(85)}  # no symbol component has these values


def _fmt(name):
    from srsran_projectvtlmo_amd import _lib
    return _lib.SYM_CI8 if name == "ci8" else _lib.SYM_CF32


def _expected(bits, mod, fmt):
    """(n, 2) array of the format's elements: float32 (compared as uint32) or int8"""
    if fmt == "ci8":
        return M.levels(bits, mod)
    return M.modulate(bits, mod).view(np.float32).reshape(-1, 2)


def _same(got, exp):
    if exp.dtype == np.float32:
        return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(exp).view(np.uint32))
    return np.array_equal(got, exp)


def _scrambled(bits, c_init, seq_offset):
    """bits ^ c(seq_offset ..): the brute-force walk, and the compiled reference's apply_xor where it was built"""
    out = bits ^ R.sequence(c_init, seq_offset, bits.size)
    if REF.available():
        ref = REF.xor_packed(np.packbits(bits), c_init, seq_offset, bits.size)
        assert np.array_equal(np.unpackbits(ref)[:bits.size], out), "reference apply_xor differs from the walk"
    return out


def _device_buffer(n_sym, fmt):
    import torch
    dt = torch.int8 if fmt == "ci8" else torch.float32
    return torch.full((n_sym, 2), float(SENTINEL[fmt]), dtype=dt, device="cuda")


def _sync(hip_ctx, bits, mod, fmt):
    from srsran_projectvtlmo_amd import channel_modulation as cm
    n = bits.size // M.qm(mod)
    mapper = cm.create_channel_modulation_hip_factory(hip_ctx).create_modulation_mapper()
    if fmt == "ci8":
        out = np.zeros((n, 2), np.int8)
        sc = mapper.modulate(out, np.packbits(bits), cm.modulation_scheme(mod))
        assert np.array([sc], np.float32).view(np.uint32)[0] == M.SCALING_BITS[mod]
        return out
    out = np.zeros(n, np.complex64)
    assert mapper.modulate(out, np.packbits(bits), cm.modulation_scheme(mod)) is None
    return out.view(np.float32).reshape(-1, 2)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mod", M.SCHEMES)
def test_all_indices(hip_ctx, mod, fmt):
    """Every symbol index in order (the two BPSKs: bits 0, 0, 1, 1, so both parities see both bits)."""
    bits = M.all_index_bits(mod)
    got, exp = _sync(hip_ctx, bits, mod, fmt), _expected(bits, mod, fmt)
    assert _same(got, exp), f"first difference at symbol {np.flatnonzero((got != exp).any(axis=1))[:1]}"


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mod", M.SCHEMES)
def test_lengths(hip_ctx, mod, fmt):
    """1, 3, 17 and 4099 symbols of random bits: a partial chunk alone, and more than one workgroup's worth ending in a
    partial last word for every Qm."""
    rng = np.random.default_rng(100 + mod)
    for n in (1, 3, 17, 4099):
        bits = rng.integers(0, 2, n * M.qm(mod)).astype(np.uint8)
        assert _same(_sync(hip_ctx, bits, mod, fmt), _expected(bits, mod, fmt)), f"{n} symbols"


# (scheme, symbols, scramble, c_init, sequence offset, input byte misalignment, symbol misalignment)
SEGMENTS = [
    (8, 70000, True, C_INIT, 0, 0, 0),             # many workgroups, vector stores
    (6, 333, True, C_INIT, 1, 1, 1),               # E = 1998 is no multiple of 8: the next segment follows its last byte
    (2, 1001, True, 0, 1998, -1, 3),               # c_init 0 is a legal seed; input directly behind the 64-QAM bits
    (4, 777, False, 0, 0, 3, 0),                   # not scrambled
    (1, 100, True, C_INIT, 31, 1, 5),
    (0, 101, True, C_INIT, 32, 2, 0),
    (8, 515, True, 0x7FFFFFFF, 33, 1, 1),
    (6, 1030, True, C_INIT, 9760 * 3, 0, 0),
    (2, 4099, True, C_INIT, (1 << 20) + 5, 3, 0),
    (4, 2050, True, C_INIT, (1 << 25) + 17, 1, 7),
    (2, 64, False, 0, 0, 0, 0),
]


@functools.lru_cache(maxsize=1)
def _segment_data():
    """The launch's layout, input bytes and scrambled bits, shared by both formats (computed once)."""
    from srsran_projectvtlmo_amd import channel_modulation as cm
    rng = np.random.default_rng(77)
    segs, parts = [], []
    bpos, spos, end = 16, 8, 0
    for mod, n, scr, c_init, so, bmis, smis in SEGMENTS:
        nbits = n * M.qm(mod)
        bits = rng.integers(0, 2, nbits).astype(np.uint8)
        a = end if bmis < 0 else bpos + bmis        # bmis < 0: directly behind the previous segment's last byte
        end = a + (nbits + 7) // 8
        bpos = (end + 15) // 16 * 16 + 16
        s = spos + smis
        spos = (s + n + 7) // 8 * 8 + 8
        segs.append(cm.mod_segment(n, mod, a, s, scr, c_init, so))
        parts.append((a, s, bits, _scrambled(bits, c_init, so) if scr else bits))
    h = rng.integers(0, 256, bpos + 16).astype(np.uint8)   # random bytes around the segments: nothing else is read
    for (a, _, bits, _), (mod, n, *_rest) in zip(parts, SEGMENTS):
        nb = bits.size // 8
        h[a:a + nb] = np.packbits(bits[:8 * nb])
        if bits.size % 8:                                   # the last byte's other bits stay random
            keep = 0xFF >> (bits.size % 8)
            h[a + nb] = (h[a + nb] & keep) | np.packbits(bits[8 * nb:])[0]
    return segs, parts, h, spos


@pytest.mark.parametrize("fmt", FORMATS)
def test_multi_segment_launch(hip_ctx, fmt):
    """One launch of eleven segments: all six schemes, odd input byte offsets, symbol offsets on and off the 16-byte
    grid, a 64-QAM segment whose bits end inside a byte followed directly by another segment, scramble on and off,
    c_init 0, sequence offsets through every radix-32 digit of the jump table, one segment of 70,000 symbols. The
    sentinel elements around and between the segments stay untouched."""
    import torch
    from srsran_projectvtlmo_amd import channel_modulation as cm
    segs, parts, h, nsym = _segment_data()
    assert segs[2].bit_offset == segs[1].bit_offset + 250  # directly behind the 64-QAM segment's last byte (1998 bits)
    d_bits = torch.from_numpy(h).cuda()
    d_sym = _device_buffer(nsym + 8, fmt)
    exp = d_sym.cpu().numpy().copy()
    for (mod, *_), (_, s, _, sbits) in zip(SEGMENTS, parts):
        e = _expected(sbits, mod, fmt)
        exp[s:s + e.shape[0]] = e
    cm.modulate_launch(hip_ctx, segs, d_bits.data_ptr(), d_sym.data_ptr(), _fmt(fmt),
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_sym.cpu().numpy()
    if fmt == "cf32":
        got, exp = got.view(np.uint32), exp.view(np.uint32)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"first difference at symbol {bad[:1]} of the buffer"


@pytest.mark.parametrize("mod", M.SCHEMES)
def test_round_trip_through_the_demodulator(hip_ctx, mod):
    """The device's cf32 symbols, no noise added, noise variance 0.01, through the oracle's soft demodulator (and the
    compiled reference's where it was built): no LLR is zero and the hard decisions are the bits."""
    rng = np.random.default_rng(200 + mod)
    n = 4096
    bits = rng.integers(0, 2, n * M.qm(mod)).astype(np.uint8)
    sym = np.ascontiguousarray(_sync(hip_ctx, bits, mod, "cf32")).view(np.complex64).reshape(-1)
    nv = np.full(n, 0.01, np.float32)
    for demod in [O.demodulate_soft] + ([REF.demodulate_soft] if REF.available() else []):
        llr = demod(mod, sym, nv)
        assert np.all(llr != 0)
        assert np.array_equal((llr < 0).astype(np.uint8), bits)


# ---- rate matching, scrambling and mapping in one launch ---------------------------------------------------------------
# (bg, Z, F, Qm, rv, Nref, [E per codeblock of one codeword])
FUSED_CASES = [
    (2, 36, 88, 2, 0, 0, [1248]),
    (1, 64, 0, 6, 2, 3000, [1998]),                 # Nref below N = 4224
    (2, 52, 0, 4, 3, 0, [2800]),                    # E above N = 2600: the selection wraps around
    (1, 384, 0, 8, 0, 0, [9728, 9760]),             # two codeblocks of one codeword: the second starts at bit 9728
    (2, 36, 40, 1, 1, 0, [777]),                    # BPSK, the fused kernel's one-bit path
]


@functools.lru_cache(maxsize=1)
def _fused_data():
    """Codewords (oracle encoder), the launch's descriptors and the scrambled rate-matched bits per codeblock."""
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    rng = np.random.default_rng(55)
    cws, rm, mods, scr_bits = [], [], [], []
    co = oo = 0
    so = 3                                           # symbol offsets: the first off the 16-byte grid
    for k, (bg, Z, F, Qm, rv, Nref, Es) in enumerate(FUSED_CASES):
        c_init = (C_INIT + k) & 0x7FFFFFFF
        seq = 0
        for E in Es:
            K, N = O.BG_K[bg], O.BG_N_SHORT[bg] * Z
            msg = rng.integers(0, 2, K * Z).astype(np.uint8)
            if F:
                msg[K * Z - F:] = O.FILLER_BIT
            cw = O.ldpc_encode(bg, Z, msg)
            e = O.rate_match(cw, E, rv, Qm, Nref, bg, Z)
            if REF.available():
                assert np.array_equal(REF.rate_match(cw, E, rv, Qm, Nref, bg, Z), e)
            cws.append((co, np.packbits(np.where(cw == O.FILLER_BIT, 0, cw).astype(np.uint8))))
            rm.append(cc.cb_rate_match_spec(N, E, Qm, rv, Nref, F, co, oo))
            mods.append(cm.mod_segment(E // Qm, Qm, oo, so, True, c_init, seq))
            scr_bits.append(_scrambled(e, c_init, seq))
            co += ((N + 7) // 8 + 15) // 16 * 16
            oo += ((E + 7) // 8 + 15) // 16 * 16
            so += E // Qm if E == 9728 else (E // Qm + 7) // 8 * 8 + 8    # the codeword's two codeblocks are contiguous
            seq += E
    h = np.zeros(co, np.uint8)
    for off, p in cws:
        h[off:off + p.size] = p
    return h, rm, mods, scr_bits, oo, so


@pytest.mark.parametrize("fmt", FORMATS)
def test_fused_rate_match_modulate(hip_ctx, fmt):
    """The fused launch against the chain oracle rate matcher -> XOR -> helper, and against the three launches on the
    device (rate_match_launch, scramble_bits_launch in place, modulate_launch), bit for bit."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import sequence_generators as sg
    h, rm, mods, scr_bits, nbytes, nsym = _fused_data()
    s = torch.cuda.current_stream().cuda_stream
    d_cw = torch.from_numpy(h).cuda()
    d_sym = _device_buffer(nsym + 8, fmt)
    exp = d_sym.cpu().numpy().copy()
    for m, b in zip(mods, scr_bits):
        exp[m.symbol_offset:m.symbol_offset + m.nof_symbols] = _expected(b, m.modulation, fmt)
    cm.rate_match_modulate_launch(hip_ctx, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), _fmt(fmt), s)
    torch.cuda.synchronize()
    got = d_sym.cpu().numpy()
    # the three-launch path
    d_bits = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_sym3 = _device_buffer(nsym + 8, fmt)
    cc.rate_match_launch(hip_ctx, rm, d_cw.data_ptr(), d_bits.data_ptr(), s)
    sg.scramble_bits_launch(hip_ctx, [sg.prs_segment(r.rm_length, m.c_init, m.seq_offset, r.out_offset, r.out_offset)
                                      for r, m in zip(rm, mods)], d_bits.data_ptr(), d_bits.data_ptr(), s)
    plain = [cm.mod_segment(m.nof_symbols, m.modulation, m.bit_offset, m.symbol_offset) for m in mods]
    cm.modulate_launch(hip_ctx, plain, d_bits.data_ptr(), d_sym3.data_ptr(), _fmt(fmt), s)
    torch.cuda.synchronize()
    got3 = d_sym3.cpu().numpy()
    if fmt == "cf32":
        got, got3, exp = got.view(np.uint32), got3.view(np.uint32), exp.view(np.uint32)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"fused: first difference at symbol {bad[:1]} of the buffer"
    bad = np.flatnonzero((got3 != exp).any(axis=1))
    assert bad.size == 0, f"three launches: first difference at symbol {bad[:1]} of the buffer"


def test_graph_replay(hip_ctx):
    """encode_launch and the fused launch recorded into one graph (launched once, then captured): the replay into a
    cleared buffer equals the eager output."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    rng = np.random.default_rng(66)
    bg, Z, Qm, E = 2, 36, 4, 1600
    K, N = O.BG_K[bg], O.BG_N_SHORT[bg] * Z
    msgs = rng.integers(0, 2, (2, K * Z)).astype(np.uint8)
    mstride, cstride = ((K * Z + 7) // 8 + 15) // 16 * 16, ((N + 7) // 8 + 15) // 16 * 16
    h = np.zeros(2 * mstride, np.uint8)
    for i in (0, 1):
        h[i * mstride:i * mstride + (K * Z + 7) // 8] = np.packbits(msgs[i])
    enc = [cc.cb_encode_spec(bg, Z, N, i * mstride, i * cstride) for i in (0, 1)]
    rm = [cc.cb_rate_match_spec(N, E, Qm, 0, 0, 0, i * cstride, 0) for i in (0, 1)]
    mods = [cm.mod_segment(E // Qm, Qm, 0, i * (E // Qm), True, C_INIT, i * E) for i in (0, 1)]
    d_msg = torch.from_numpy(h).cuda()
    d_cw = torch.zeros(2 * cstride, dtype=torch.uint8, device="cuda")
    d_sym = _device_buffer(2 * (E // Qm), "cf32")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def chain():
        cc.encode_launch(hip_ctx, enc, d_msg.data_ptr(), d_cw.data_ptr(), st.cuda_stream)
        cm.rate_match_modulate_launch(hip_ctx, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), _fmt("cf32"),
                                      st.cuda_stream)
    chain()
    st.synchronize()
    eager = d_sym.cpu().numpy().copy()
    exp = np.concatenate([_expected(_scrambled(O.rate_match(O.ldpc_encode(bg, Z, msgs[i]), E, 0, Qm, 0, bg, Z),
                                               C_INIT, i * E), Qm, "cf32") for i in (0, 1)])
    assert _same(eager, exp)
    L, graph = hip_ctx.lib, ctypes.c_void_p()
    assert L.ldpc_hip_capture_begin(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream)) == 0
    chain()
    assert L.ldpc_hip_capture_end(hip_ctx.handle, ctypes.c_void_p(st.cuda_stream), ctypes.byref(graph)) == 0
    d_sym.fill_(float(SENTINEL["cf32"]))
    d_cw.zero_()
    torch.cuda.synchronize()
    assert L.ldpc_hip_graph_launch(graph, ctypes.c_void_p(st.cuda_stream)) == 0
    st.synchronize()
    replay = d_sym.cpu().numpy()
    L.ldpc_hip_graph_destroy(graph)
    assert _same(replay, eager)


# ---- loopback: device downlink chain into the device uplink slot -------------------------------------------------------
LOOP_UES = [(256, 2, 156 * 4, "QPSK", 4), (3000, 2, 1500, "QAM16", 2), (9000, 1, 3000, "QAM64", 2),
            (20000, 1, 7000, "QAM256", 4)]
LOOP_IDS = [(0x1234, 0x155), (1, 0), (65535, 1023), (0x4601, 7)]  # (rnti, n_id) per TB


def test_loopback_through_the_slot_pipeline(hip_ctx):
    """Four small TBs encoded, rate-matched, scrambled and mapped on the device (encode_launch, the fused launch), the
    cf32 symbols handed, with no noise added and noise variance 0.01, to the PUSCH slot pipeline with the matching
    scrambling entries: every TB CRC passes and the TB bytes are the data."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import pusch
    from srsran_projectvtlmo_amd.sequence_generators import pusch_c_init
    rng = np.random.default_rng(91)
    tbs = [TransportBlock(rng, *ue) for ue in LOOP_UES]
    enc, rm, mods, msgs = [], [], [], []
    mo = co = so = 0
    tb_sym = []
    for tb, (rnti, n_id) in zip(tbs, LOOP_IDS):
        seq, first = 0, so
        for r, m in enumerate(tb.metas):
            E = m["rm_length"]
            msgs.append((mo, np.packbits(np.where(tb.msgs[r] == O.FILLER_BIT, 0, tb.msgs[r]).astype(np.uint8))))
            enc.append(cc.cb_encode_spec(tb.bg, tb.Z, tb.N, mo, co))
            rm.append(cc.cb_rate_match_spec(tb.N, E, tb.Qm, 0, 0, tb.F, co, 0))
            mods.append(cm.mod_segment(E // tb.Qm, tb.Qm, 0, so, True, pusch_c_init(rnti, n_id), seq))
            mo += ((tb.K * tb.Z + 7) // 8 + 15) // 16 * 16
            co += ((tb.N + 7) // 8 + 15) // 16 * 16
            so += E // tb.Qm
            seq += E
        tb_sym.append((first, so))
    h = np.zeros(mo, np.uint8)
    for off, p in msgs:
        h[off:off + p.size] = p
    s = torch.cuda.current_stream().cuda_stream
    d_msg = torch.from_numpy(h).cuda()
    d_cw = torch.zeros(co, dtype=torch.uint8, device="cuda")
    d_sym = torch.zeros(so, dtype=torch.complex64, device="cuda")
    cc.encode_launch(hip_ctx, enc, d_msg.data_ptr(), d_cw.data_ptr(), s)
    cm.rate_match_modulate_launch(hip_ctx, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), _fmt("cf32"), s)
    specs = [pusch.tb_slot_spec(tb.tbs, tb.bg, tb.Z, tb.F, [m["rm_length"] for m in tb.metas], tb.Qm, 0, True, 0, 6,
                                True, rnti=rnti, n_id=n_id) for tb, (rnti, n_id) in zip(tbs, LOOP_IDS)]
    pipe = pusch.SlotPipeline(hip_ctx, specs)
    assert pipe.scrambled
    pipe.upload_symbols_device([d_sym[a:b] for a, b in tb_sym],
                               [torch.full((b - a,), 0.01, dtype=torch.float32, device="cuda") for a, b in tb_sym])
    pipe.launch(s)
    torch.cuda.synchronize()
    got, _ = pipe.results()
    for t, (tb, (tb_bytes, ok, _w)) in enumerate(zip(tbs, got)):
        assert ok, f"tb {t}: TB CRC"
        assert np.array_equal(np.unpackbits(tb_bytes)[:tb.tbs], tb.data), f"tb {t}: bytes"


# ---- refused calls ---------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(hip_ctx):
    """Every LDPC_HIP_EINVAL case returns it with a message and leaves the output untouched."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_modulation as cm
    L, c = hip_ctx.lib, hip_ctx.handle
    d_bits = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_sym = _device_buffer(4096, "ci8")
    bits, sym = ctypes.c_void_p(d_bits.data_ptr()), ctypes.c_void_p(d_sym.data_ptr())
    ok = cm.mod_descriptors([cm.mod_segment(64, 4)])
    rm = (_lib.RmDesc * 1)()
    rm[0].cb_length, rm[0].rm_length, rm[0].modulation_order = 50 * 36, 256, 4

    def refused(rc, word):
        assert rc == _lib.EINVAL
        msg = L.ldpc_hip_last_error(c)
        assert word in msg, msg

    refused(L.ldpc_hip_modulate_launch(c, 1, cm.mod_descriptors([cm.mod_segment(64, 3)]), bits, sym, 1, None),
            b"scheme")
    refused(L.ldpc_hip_modulate_launch(c, 1, ok, bits, sym, 2, None), b"format")
    refused(L.ldpc_hip_modulate_launch(c, 1, ok, None, sym, 1, None), b"null")
    refused(L.ldpc_hip_modulate_launch(c, 1, ok, bits, None, 1, None), b"null")
    refused(L.ldpc_hip_modulate_launch(c, 1, None, bits, sym, 1, None), b"null")
    refused(L.ldpc_hip_modulate_launch(c, 1, cm.mod_descriptors([cm.mod_segment(64, 4, 0, 0, True, 1 << 31)]), bits,
                                       sym, 1, None), b"c_init")
    refused(L.ldpc_hip_modulate_launch(c, 1, cm.mod_descriptors([cm.mod_segment(1 << 31, 8)]), bits, sym, 1, None),
            b"2^31")
    host = np.full((64, 2), 85, np.int8)
    refused(L.ldpc_hip_modulate_sync(c, 64, 3, host.ctypes.data, host.ctypes.data, 1), b"scheme")
    refused(L.ldpc_hip_modulate_sync(c, 64, 4, host.ctypes.data, host.ctypes.data, 7), b"format")
    refused(L.ldpc_hip_modulate_sync(c, 64, 4, None, host.ctypes.data, 1), b"null")
    assert np.all(host == 85)
    # the fused launch: a good pair first, then each contract violation
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, cm.mod_descriptors([cm.mod_segment(63, 4)]), bits, sym, 1,
                                                  None), b"rm_length")
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, cm.mod_descriptors([cm.mod_segment(128, 2)]), bits, sym, 1,
                                                  None), b"modulation_order")
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, cm.mod_descriptors([cm.mod_segment(64, 9)]), bits, sym, 1,
                                                  None), b"scheme")
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, ok, bits, sym, 5, None), b"format")
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, ok, None, sym, 1, None), b"null")
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, None, bits, sym, 1, None), b"null")
    rm[0].rm_length, rm[0].modulation_order = 64, 1
    refused(L.ldpc_hip_rate_match_modulate_launch(c, 1, rm, cm.mod_descriptors([cm.mod_segment(64, 0)]), bits, sym, 1,
                                                  None), b"pi/2-BPSK")
    # zero counts need no buffers
    assert L.ldpc_hip_modulate_launch(c, 0, None, None, None, 1, None) == 0
    assert L.ldpc_hip_rate_match_modulate_launch(c, 0, None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert np.all(d_sym.cpu().numpy() == 85), "a refused launch wrote symbols"
