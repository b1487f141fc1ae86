"""GPU tests of the PDSCH encoder plugin (hal::hw_accelerator_pdsch_enc on the MI355X, ldpc_hip_enc_* C ABI) driven in
pdsch_encoder_hw_impl's call order (tests/pdsch_flow.py), bit-exact against the oracle's TB CRC -> segmentation ->
CB CRC -> LDPC encoder -> rate matcher chain. Mirrors the reference's pdsch_encoder_test.cpp (which checks the HW
encoder against the same software chain) and pdsch_encoder_hwacc_benchmark.cpp's TB / CB modes."""
import numpy as np
import pytest

from tests.pdsch_flow import encode_hw, expected_codeword

pytestmark = pytest.mark.gpu

# (tbs, bg, nof_ch_symbols, modulation, layers, rv, Nref)
CASES = [
    (256, 2, 156 * 4, "QPSK", 4, 0, 0),                 # C4's small UEs: one BG2 Z=36 codeblock, CRC16, filler
    (1078248, 1, 250 * 156 * 4, "QAM256", 4, 0, 0),     # C4's UE0: 128 BG1 Z=384 codeblocks
    (40000, 2, 52 * 156, "QAM64", 2, 2, 0),             # 11 BG2 codeblocks, rv 2 (ldpc_segmenter_test_data.h case)
    (8456, 1, 24 * 156 + 2, "QPSK", 1, 3, 0),           # 2 BG1 codeblocks, rv 3, E = 3746 (not a multiple of 8)
    (30000, 1, 40 * 156, "QPSK", 2, 1, 25344 // 2),     # limited buffer (Nref), rv 1
    (1024, 2, 12 * 156, "BPSK", 1, 0, 0),               # BPSK, one codeblock, CRC16
]


@pytest.fixture(scope="module")
def ctx():
    from srsran_projectvtlmo_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _tb(rng, tbs):
    return rng.integers(0, 256, tbs // 8).astype(np.uint8)


@pytest.mark.parametrize("cb_mode", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[f"tbs{c[0]}_bg{c[1]}_{c[3]}" for c in CASES])
def test_pdsch_encoder_plugin_bit_exact(ctx, case, cb_mode):
    from srsran_projectvtlmo_amd import hal
    tbs, bg, nsym, mod, layers, rv, Nref = case
    rng = np.random.default_rng(tbs + 7 * bg + rv)
    tb = _tb(rng, tbs)
    enc = hal.hw_accelerator_pdsch_enc_hip(ctx, cb_mode=cb_mode)
    try:
        assert enc.get_cb_mode() == cb_mode
        got, stats = encode_hw(enc, tb, bg, nsym, mod, layers, rv, Nref)
    finally:
        enc.close()
    want = expected_codeword(tb, bg, nsym, mod, layers, rv, Nref)
    assert stats["enqueue_false"] == 0
    np.testing.assert_array_equal(got, want)


def test_pdsch_encoder_queue_full_and_tb_size_limit(ctx):
    """A batch of 16 codeblocks: a 41-CB TB in CB mode fills it (enqueue_operation returns False, the caller dequeues
    and enqueues the rest: three batches); in TB mode a TB above get_max_tb_size() is encoded in CB mode
    (pdsch_encoder_hw_impl.cpp:35-40). Both bit-exact."""
    from srsran_projectvtlmo_amd import hal
    rng = np.random.default_rng(40)
    tbs, bg, nsym, mod, layers = 337920, 1, 200 * 156, "QAM64", 4   # 41 BG1 codeblocks
    tb = _tb(rng, tbs)
    want = expected_codeword(tb, bg, nsym, mod, layers, 0, 0)
    enc = hal.hw_accelerator_pdsch_enc_hip(ctx, cb_mode=True, max_queue_cbs=16)
    try:
        got, stats = encode_hw(enc, tb, bg, nsym, mod, layers, 0, 0)
    finally:
        enc.close()
    np.testing.assert_array_equal(got, want)
    assert stats["enqueue_false"] == 2 and stats["batches"] == 3
    enc = hal.hw_accelerator_pdsch_enc_hip(ctx, cb_mode=False, max_tb_bytes=4096)
    try:
        assert enc.get_max_tb_size() == 4096 and not enc.get_cb_mode()
        got, _ = encode_hw(enc, tb, bg, nsym, mod, layers, 0, 0)
    finally:
        enc.close()
    np.testing.assert_array_equal(got, want)


def test_pdsch_encoder_factory_and_contract(ctx):
    """The factory selects the plugin by acc_type (hw_accelerator_factories.cpp); calls out of order and invalid
    configurations are refused, as the reference asserts."""
    from srsran_projectvtlmo_amd import _lib, hal
    assert hal.create_hw_accelerator_pdsch_enc_factory(hal.hw_accelerator_pdsch_enc_configuration(acc_type="acc100")) \
        is None
    f = hal.create_hw_accelerator_pdsch_enc_factory(hal.hw_accelerator_pdsch_enc_configuration(cb_mode=True))
    enc = f.create()
    try:
        assert enc.get_cb_mode() and enc.get_max_tb_size() == 159749
        cfg = hal.hw_pdsch_encoder_configuration(nof_tb_bits=256, base_graph_index=2, modulation="QPSK",
                                                 nof_segments=1, lifting_size=36, Ncb=1800, nof_filler_bits=88,
                                                 rm_length=1248, cb_mode=True)
        with pytest.raises(_lib.LdpcHipError):          # enqueue before reserve_queue
            enc.configure_operation(cfg, 0)
            enc.enqueue_operation(np.zeros((360 - 88 + 7) // 8, np.uint8), None, 0)
        enc.reserve_queue()
        bad = hal.hw_pdsch_encoder_configuration(**{**cfg.__dict__, "rm_length": 1249})  # E not a multiple of Qm
        with pytest.raises(_lib.LdpcHipError):
            enc.configure_operation(bad, 0)
        enc.configure_operation(cfg, 0)
        with pytest.raises(_lib.LdpcHipError):          # wrong data size
            enc.enqueue_operation(np.zeros(5, np.uint8), None, 0)
        assert enc.enqueue_operation(np.zeros((360 - 88 + 7) // 8, np.uint8), None, 0)
        out = np.zeros(1248, np.uint8)
        while not enc.dequeue_operation(out, None, 0):
            pass
        enc.free_queue()
    finally:
        enc.close()
        enc.ctx.close()


# Small batches (<= 8 codeblocks) take the encoder's device work queue (ldpc_dwq_encode_kernel); a context with
# LDPC_HIP_LAUNCH_NO_DWQ launches ldpc_pdsch_encode_kernel instead. Both routes, both modes, against the oracle chain;
# the 6-CB BG2 TB has segments of 3,338 bits, so TB mode reads them at bit offsets and attaches their CRC24B on the
# device.
SMALL_CASES = [
    (256, 2, 156 * 4, "QPSK", 4, 0, 0),        # one BG2 Z=36 codeblock, CRC16, filler
    (8456, 1, 24 * 156 + 2, "QPSK", 1, 3, 0),  # 2 BG1 codeblocks, rv 3
    (20000, 2, 52 * 156, "QAM64", 2, 1, 0),    # 6 BG2 codeblocks, segments not byte aligned, rv 1
]


@pytest.mark.parametrize("route", ["work_queue", "launch"])
@pytest.mark.parametrize("cb_mode", [False, True])
@pytest.mark.parametrize("case", SMALL_CASES, ids=[f"tbs{c[0]}_bg{c[1]}_{c[3]}" for c in SMALL_CASES])
def test_pdsch_encoder_small_batches_both_routes(case, cb_mode, route):
    from srsran_projectvtlmo_amd import _lib, hal
    tbs, bg, nsym, mod, layers, rv, Nref = case
    rng = np.random.default_rng(tbs + 11 * bg + rv)
    tb = _tb(rng, tbs)
    c = _lib.Context(0, launch_flags=_lib.LAUNCH_NO_DWQ if route == "launch" else 0)
    try:
        enc = hal.hw_accelerator_pdsch_enc_hip(c, cb_mode=cb_mode)
        try:
            got, stats = encode_hw(enc, tb, bg, nsym, mod, layers, rv, Nref)
        finally:
            enc.close()
    finally:
        c.close()
    assert stats["enqueue_false"] == 0
    np.testing.assert_array_equal(got, expected_codeword(tb, bg, nsym, mod, layers, rv, Nref))


# ---- TB mode: the message edges of enc_build -----------------------------------------------------------------------
# ldpc_hip_enc_configure takes any TB-mode configuration with nof_segment_bits + 24 + F == K Z (C > 1) and S C >= B, so
# these are built directly, not through the segmenter. In TB mode the device reads segment r at bit r S of TB + TB CRC
# (byte r S / 8, bit offset r S % 8), zero-pads it to S bits, and attaches its CRC24B at bit S: word S / 32, shift
# S % 32, spilling into the next word for a shift above 8; the CRC runs over ceil(S / 32) front-padded words, one per
# thread and round of 256.
# (name, bg, Z, S, C, TB bits, TB CRC bits)
TB_EDGE_CASES = [
    # C = 8 segments of an odd length: they start at all eight bit offsets
    ("bit_offsets_bg2_z36", 2, 36, 335, 8, 8 * 335 - 16, 16),
    ("bit_offsets_bg1_z104", 1, 104, 2263, 8, 8 * 2263 - 24, 24),
] + [
    # the CRC's place in its word: S % 32 = 0, below 8, at 8, above (the spill), up to 31
    (f"crc_at_{S % 32}", 2, 36, S, 2, (2 * S - 16) // 8 * 8, 16) for S in (288, 289, 295, 296, 297, 312, 313, 319)
] + [
    ("crc_one_word_s20", 2, 6, 20, 2, 24, 16),            # CRC over at most 32 bits: one front-padded word
    ("crc_one_word_s32", 2, 6, 32, 2, 48, 16),
    ("crc_two_rounds", 1, 384, 8424, 2, 2 * 8424 - 24, 24),   # 264 CRC words: more than one per thread
    ("short_last_segment", 2, 36, 300, 3, 656, 24),       # B = 680: the last segment holds 80 of 300 bits
    ("segment_past_the_end", 2, 36, 300, 4, 656, 24),     # and a fourth one holds none
    ("segment_starts_at_the_end", 2, 36, 300, 3, 576, 24),    # B = 600 = 2 S: the third starts where the TB ends
]


def _tb_edge_expected(bg, Z, S, C, tb_bits, L, Qm, rv, Ea, Eb, nshort):
    import oracle as O
    from tests.pdsch_flow import cb_messages
    KZ = O.BG_K[bg] * Z
    F = KZ - 24 - S
    msgs = cb_messages(tb_bits, bg=bg, Z=Z, seg_bits=S, C=C, F=F, tb_crc_bits=L)
    # cb_messages' slicing and CRC placement, restated from the TB's bits: segment r is bits [r S, r S + n) of TB + TB
    # CRC and zeros up to S, its CRC24B (the packed-bytes routine, not the one cb_messages calls) sits at [S, S + 24)
    tcrc = O.crc_bits(O.CRC16 if L == 16 else O.CRC24A, tb_bits)
    b = np.concatenate([tb_bits, [(tcrc >> (L - 1 - i)) & 1 for i in range(L)]]).astype(np.uint8)
    B = b.size
    for r in range(C):
        n = max(0, min(S, B - r * S))
        seg = np.zeros(S, np.uint8)
        seg[:n] = b[r * S:r * S + n]
        assert np.array_equal(msgs[r, :S], seg)
        crc = O.crc_packed(O.CRC24B, np.packbits(seg), S)
        assert np.array_equal(msgs[r, S:S + 24], [(crc >> (23 - i)) & 1 for i in range(24)])
        assert np.all(msgs[r, KZ - F:] == O.FILLER_BIT)
        if n == 0:
            assert crc == 0 and not np.any(msgs[r, :KZ - F])    # a segment past the end: all zero, zero CRC
    return [O.rate_match(O.ldpc_encode(bg, Z, msgs[r]), Ea if r < nshort else Eb, rv, Qm, 0, bg, Z) for r in range(C)]


@pytest.mark.parametrize("route", ["work_queue", "launch"])
@pytest.mark.parametrize("case", TB_EDGE_CASES, ids=[c[0] for c in TB_EDGE_CASES])
def test_pdsch_encoder_tb_mode_message_edges(case, route):
    import oracle as O
    from srsran_projectvtlmo_amd import _lib, hal
    name, bg, Z, S, C, tbs, L = case
    k = [c[0] for c in TB_EDGE_CASES].index(name)
    KZ, N = O.BG_K[bg] * Z, O.BG_N_SHORT[bg] * Z
    F = KZ - 24 - S
    B = tbs + L
    assert tbs % 8 == 0 and 0 <= F < (O.BG_K[bg] - 2) * Z and S * C >= B
    if name.startswith("bit_offsets"):
        assert {(r * S) % 8 for r in range(C)} == set(range(8)) and B == S * C
    segs = [max(0, min(S, B - r * S)) for r in range(C)]
    assert any(0 < n < S for n in segs) or not ("short" in name or "past" in name)
    assert ("past" in name or "starts_at" in name) == (0 in segs)
    rng = np.random.default_rng(500 + k)
    tb = _tb(rng, tbs)
    tb_bits = np.unpackbits(tb)
    Qm, mod, rv = (2, "QPSK", k % 4) if k % 2 else (6, "QAM64", k % 4)
    Ea = (N // 2 + 7 * k) // Qm * Qm
    Eb, nshort = Ea + Qm, C // 2
    want = _tb_edge_expected(bg, Z, S, C, tb_bits, L, Qm, rv, Ea, Eb, nshort)
    crc = O.crc_bits(O.CRC16 if L == 16 else O.CRC24A, tb_bits)
    cfg = hal.hw_pdsch_encoder_configuration(
        nof_tb_bits=tbs, nof_tb_crc_bits=L, base_graph_index=bg, modulation=mod, nof_segments=C,
        nof_short_segments=nshort, rv=rv, cw_length_a=Ea, cw_length_b=Eb, lifting_size=Z, Ncb=N, Nref=0,
        nof_segment_bits=S, nof_filler_bits=F, rm_length=Ea,
        tb_crc=tuple((crc >> s) & 0xff for s in ((16, 8, 0) if L == 24 else (8, 0))), cb_mode=False)
    total = sum(w.size for w in want)
    block = np.full(total, 0xEE, np.uint8)
    packed = np.full(sum((w.size + 7) // 8 for w in want), 0xEE, np.uint8)
    c = _lib.Context(0, launch_flags=_lib.LAUNCH_NO_DWQ if route == "launch" else 0)
    try:
        enc = hal.hw_accelerator_pdsch_enc_hip(c, cb_mode=False)
        try:
            enc.reserve_queue()
            enc.configure_operation(cfg, 0)
            assert enc.enqueue_operation(tb, None, 0)
            while not enc.dequeue_operation(block, packed, 0):
                pass
            enc.free_queue()
        finally:
            enc.close()
    finally:
        c.close()
    o = 0
    for r, w in enumerate(want):
        assert np.array_equal(block[o:o + w.size], w), f"segment {r} of {C} ({segs[r]} of {S} bits, starts at bit " \
                                                       f"{(r * S) % 8} of its byte) differs from the oracle"
        o += w.size
    np.testing.assert_array_equal(packed, np.concatenate([np.packbits(w) for w in want]))
