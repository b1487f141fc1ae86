"""GPU parity tests of the HIP LDPC decoder against the CPU oracle (bit-exact: packed message bytes, CRC status,
iteration count). Procedures follow the reference's own tests:
  * ldpc_enc_dec_test.cpp:287-331  encode -> LLR +-10 (filler +10) -> decode -> message equality, lengths
                                   create_range((K+2)Z, N_short Z, 3) incl. non-multiples of Z
  * ldpc_enc_dec_test.cpp:334-358  all-zero and almost-zero LLRs -> all-ones message, nullopt
  * ldpc_decoder_benchmark.cpp:33,144-145  random +-10 LLRs (mt19937-like distribution), 8 iterations
All calls go through the C ABI (libsrsran_ldpc_hip.so)."""
import numpy as np
import pytest

import oracle as O
from tests.vectors import codeword_llrs, msg_bits_match, random_llrs

pytestmark = pytest.mark.gpu


def _cc():
    from srsran_projectvtlmo_amd import channel_coding as cc
    return cc


def _cfg(cc, bg, Z, iters, F=0, sf=0.8):
    cfg = cc.configuration()
    cfg.block_conf.tb_common.base_graph = bg
    cfg.block_conf.tb_common.lifting_size = Z
    cfg.block_conf.cb_specific.nof_filler_bits = F
    cfg.algorithm_conf.max_iterations = iters
    cfg.algorithm_conf.scaling_factor = sf
    return cfg


CRC_NAME = {O.CRC16: "CRC16", O.CRC24B: "CRC24B", O.CRC24A: "CRC24A"}
HIP_CRC = {O.NO_CRC: -1, O.CRC16: 0, O.CRC24B: 1, O.CRC24A: 2}  # oracle numbering -> hw_dec_cb_crc_type


def _decode_both(cc, dec, bg, Z, llr, iters, crc=None, F=0, sf=0.8):
    nb = (O.BG_K[bg] * Z + 7) // 8
    out_hip = np.full(nb, 0xA5, dtype=np.uint8)
    out_orc = np.full(nb, 0xA5, dtype=np.uint8)
    crc_obj = None if crc is None else cc.crc_calculator(CRC_NAME[crc])
    r_hip = dec.decode(out_hip, llr, crc_obj, _cfg(cc, bg, Z, iters, F, sf))
    _, r_orc = O.ldpc_decode(bg, Z, llr, iters, O.NO_CRC if crc is None else crc, F, sf, out=out_orc)
    return out_hip, r_hip, out_orc, r_orc


def _create_range(lo, hi, n):
    # tests/unittests/.../ldpc_enc_dec_test.cpp create_range: n evenly spaced values from lo to hi
    if n == 1:
        return [lo]
    step = (hi - lo) // (n - 1)
    return [lo + i * step for i in range(n - 1)] + [hi]


@pytest.mark.parametrize("bg,Z", [(1, 2), (1, 7), (1, 36), (1, 384), (2, 3), (2, 52), (2, 208), (2, 384),
                                  (1, 15), (2, 11), (1, 104), (2, 240)])
def test_random_llrs_bit_exact(bg, Z):
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    rng = np.random.default_rng(1000 + 7 * Z + bg)
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    for length in _create_range((K + 2) * Z, Ns * Z, 3) + [(K + 2) * Z + 1, Ns * Z - 1]:
        for kind in ("pm10", "mixed"):
            llr = random_llrs(rng, length, kind)
            for iters in (1, 3):
                out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, iters)
                assert r_hip == r_orc is None
                np.testing.assert_array_equal(out_hip, out_orc, err_msg=f"bg{bg} Z{Z} L{length} {kind} it{iters}")


@pytest.mark.parametrize("bg,Z", [(1, 52), (2, 52), (1, 384), (2, 208)])
def test_trailing_zeros_adapt_layers(bg, Z):
    """Layer count adapts to the last non-zero LLR (ldpc_decoder_impl.cpp:85-114)."""
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    rng = np.random.default_rng(77 + Z)
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    for nz in (0, 5 * Z + 3, (Ns - K - 6) * Z):
        llr = random_llrs(rng, Ns * Z, "mixed")
        if nz:
            llr[-nz:] = 0
        out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 4)
        np.testing.assert_array_equal(out_hip, out_orc)


@pytest.mark.parametrize("bg,Z,F", [(2, 52, 0), (1, 384, 0), (2, 208, 24), (1, 36, 40), (2, 7, 6)])
def test_encode_decode_round_trip(bg, Z, F):
    """ldpc_enc_dec_test.cpp:287-331: +-10 LLRs from the codeword (filler -> +10), 1 iteration, no CRC."""
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    rng = np.random.default_rng(5 + Z)
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    msg = rng.integers(0, 2, K * Z).astype(np.uint8)
    if F:
        msg[K * Z - F:] = O.FILLER_BIT
    cw = O.ldpc_encode(bg, Z, msg)
    for length in _create_range((K + 2) * Z, Ns * Z, 3):
        llr = np.where(cw[:length] == 1, -10, 10).astype(np.int8)
        out_hip, r_hip, out_orc, _ = _decode_both(cc, dec, bg, Z, llr, 1, F=F)
        np.testing.assert_array_equal(out_hip, out_orc)
        assert msg_bits_match(out_hip, msg, K * Z)


@pytest.mark.parametrize("bg,Z", [(1, 384), (2, 52), (2, 3)])
def test_all_zero_and_almost_zero(bg, Z):
    """ldpc_enc_dec_test.cpp:334-358."""
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    KZ = K * Z
    llr = np.zeros(Ns * Z, dtype=np.int8)
    out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 6)
    assert r_hip is None and r_orc is None
    np.testing.assert_array_equal(out_hip, out_orc)
    assert np.all(np.unpackbits(out_hip)[:KZ] == 1)
    # with a CRC the output is left untouched (impl.cpp:86-94)
    out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 6, crc=O.CRC24B)
    assert r_hip is None and r_orc is None
    assert np.all(out_hip == 0xA5) and np.all(out_orc == 0xA5)
    llr = np.zeros(Ns * Z, dtype=np.int8)
    for i in range((K + 2) * Z + 2, Ns * Z, 3):
        llr[i] = 1 if i % 2 == 0 else -1
    out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 6)
    np.testing.assert_array_equal(out_hip, out_orc)
    assert np.all(np.unpackbits(out_hip)[:KZ] == 1)


@pytest.mark.parametrize("bg,Z,crc,F", [(2, 208, O.CRC24B, 0), (1, 384, O.CRC24B, 0), (2, 52, O.CRC16, 0),
                                        (1, 160, O.CRC24A, 32), (2, 36, O.CRC16, 88), (1, 11, O.CRC24B, 10)])
def test_early_stop_crc(bg, Z, crc, F):
    """CRC early termination: iteration count and CRC status equal the oracle's (impl.cpp:125-146)."""
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    rng = np.random.default_rng(900 + Z)
    seen = set()
    for noise in (0.3, 0.8, 1.0, 1.2, 1.6):
        for _ in range(3):
            llr, msg = codeword_llrs(rng, bg, Z, 2.0, noise, F=F, crc=crc)
            out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 10, crc=crc, F=F)
            assert r_hip == r_orc, f"noise {noise}"
            np.testing.assert_array_equal(out_hip, out_orc)
            seen.add(r_hip)
    assert len(seen) > 1  # both early-stopped and failed / different iteration counts were exercised


def test_scaling_factor_variants():
    cc = _cc()
    dec = cc.create_ldpc_decoder_factory_sw("hip").create()
    rng = np.random.default_rng(3)
    for sf in (0.5, 0.75, 0.9, 0.3333):
        llr = random_llrs(rng, 50 * 52, "uniform")
        out_hip, _, out_orc, _ = _decode_both(cc, dec, 2, 52, llr, 5, sf=sf)
        np.testing.assert_array_equal(out_hip, out_orc)
    # added: BG1's degree-19 rows, one-wave and multi-wave graphs, +-127 and zeros, fillers and a CRC, 0.05 (every
    # check-to-variable message 0) and 0.99; all graphs at recorded reference outputs: test_gpu_reference_fixtures.py
    for bg, Z, sf, crc, F in [(1, 384, 0.5, None, 0), (1, 36, 0.9, O.CRC24B, 26), (2, 208, 0.3333, O.CRC16, 0),
                              (1, 7, 0.75, None, 0), (1, 104, 0.05, None, 0), (2, 384, 0.99, O.CRC24A, 200)]:
        llr = random_llrs(rng, O.BG_N_SHORT[bg] * Z - 3, "mixed")
        if F:
            llr[(O.BG_K[bg] - 2) * Z - F:(O.BG_K[bg] - 2) * Z] = 127
        out_hip, r_hip, out_orc, r_orc = _decode_both(cc, dec, bg, Z, llr, 3, crc=crc, F=F, sf=sf)
        assert r_hip == r_orc, f"BG{bg} Z={Z} sf={sf}"
        np.testing.assert_array_equal(out_hip, out_orc, err_msg=f"BG{bg} Z={Z} sf={sf}")


def test_batch_plan_mixed_configs(hip_ctx):
    """DecodePlan (device pointers, one launch per (BG, Z) group) on a mixed batch, results in input order."""
    import torch
    cc = _cc()
    rng = np.random.default_rng(11)
    cases = [(1, 384, 8, O.NO_CRC, 0), (2, 36, 8, O.CRC16, 88), (2, 208, 10, O.CRC24B, 0), (1, 384, 8, O.CRC24B, 0),
             (2, 52, 6, O.NO_CRC, 0), (1, 20, 5, O.CRC24A, 8), (2, 36, 8, O.CRC16, 88)] * 3
    specs, llrs, expect = [], [], []
    llr_off = out_off = 0
    for (bg, Z, it, crc, F) in cases:
        llr, _ = codeword_llrs(rng, bg, Z, 2.0, 0.9, F=F, crc=None if crc == O.NO_CRC else crc)
        mode = cc.CRC_MODE_NONE if crc == O.NO_CRC else cc.CRC_MODE_EARLY_STOP
        specs.append(cc.cb_decode_spec(bg, Z, llr.size, it, mode, HIP_CRC[crc], F, 0.8, llr_off, out_off))
        llrs.append((llr_off, llr))
        expect.append(O.ldpc_decode(bg, Z, llr, it, crc, F))
        llr_off += (llr.size + 15) // 16 * 16
        out_off += (cc.message_bytes(bg, Z) + 15) // 16 * 16
    h_llr = np.zeros(llr_off, dtype=np.int8)
    for off, l in llrs:
        h_llr[off:off + l.size] = l
    d_llr = torch.from_numpy(h_llr).cuda()
    d_out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(len(specs) * 4, dtype=torch.uint8, device="cuda")
    plan = cc.DecodePlan(hip_ctx, specs)
    plan.launch(d_llr.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    res = d_res.cpu().numpy().reshape(-1, 4)
    for i, (s, (eo, er)) in enumerate(zip(specs, expect)):
        nb = cc.message_bytes(s.base_graph, s.lifting_size)
        np.testing.assert_array_equal(out[s.out_offset:s.out_offset + nb], eo, err_msg=f"cb {i}")
        assert (res[i, 0] == 1) == (er is not None)
        if er is not None:
            assert res[i, 1] == er


def test_c2_batch_128_bit_exact_sample(hip_ctx):
    """C2 shape (BG1 Z=384, 128 CBs, 8 iterations, +-10 LLRs): a full batch on the GPU, every CB checked."""
    import torch
    cc = _cc()
    rng = np.random.default_rng(0)
    n = 128
    specs, llr_stride, out_stride = cc.uniform_batch_specs(n, 1, 384, 8)
    h_llr = np.zeros(n * llr_stride, dtype=np.int8)
    for i in range(n):
        h_llr[i * llr_stride:i * llr_stride + 25344] = random_llrs(rng, 25344, "pm10")
    d_llr = torch.from_numpy(h_llr).cuda()
    d_out = torch.zeros(n * out_stride, dtype=torch.uint8, device="cuda")
    plan = cc.DecodePlan(hip_ctx, specs)
    plan.launch(d_llr.data_ptr(), d_out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for i in range(n):
        eo, _ = O.ldpc_decode(1, 384, h_llr[i * llr_stride:i * llr_stride + 25344], 8)
        np.testing.assert_array_equal(out[i * out_stride:i * out_stride + 1056], eo, err_msg=f"cb {i}")


def _run_plan(hip_ctx, cc, cases, llr_skew=None):
    """cases: list of (bg, Z, iters, crc, F, llr). One DecodePlan over all of them; returns (out bytes, results).
    Each codeblock's LLRs start at a multiple of 16 bytes, plus llr_skew[i] when given."""
    import torch
    specs, offs = [], []
    llr_off = out_off = 0
    for i, (bg, Z, it, crc, F, llr) in enumerate(cases):
        skew = llr_skew[i] if llr_skew is not None else 0
        mode = cc.CRC_MODE_NONE if crc == O.NO_CRC else cc.CRC_MODE_EARLY_STOP
        specs.append(cc.cb_decode_spec(bg, Z, llr.size, it, mode, HIP_CRC[crc], F, 0.8, llr_off + skew, out_off))
        offs.append(llr_off + skew)
        llr_off += (skew + llr.size + 15) // 16 * 16
        out_off += (cc.message_bytes(bg, Z) + 15) // 16 * 16
    h_llr = np.zeros(llr_off, dtype=np.int8)
    for off, c in zip(offs, cases):
        h_llr[off:off + c[5].size] = c[5]
    d_llr = torch.from_numpy(h_llr).cuda()
    d_out = torch.zeros(out_off, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(len(specs) * 4, dtype=torch.uint8, device="cuda")
    plan = cc.DecodePlan(hip_ctx, specs)
    plan.launch(d_llr.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.close()
    return specs, d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 4)


def _check_against_oracle(cc, specs, cases, out, res):
    for i, (s, (bg, Z, it, crc, F, llr)) in enumerate(zip(specs, cases)):
        eo, er = O.ldpc_decode(bg, Z, llr, it, crc, F)
        nb = cc.message_bytes(bg, Z)
        np.testing.assert_array_equal(out[s.out_offset:s.out_offset + nb], eo, err_msg=f"cb {i} BG{bg} Z={Z}")
        assert (res[i, 0] == 1) == (er is not None), f"cb {i} BG{bg} Z={Z}"
        if er is not None:
            assert res[i, 1] == er, f"cb {i} BG{bg} Z={Z}"


def test_every_lifted_graph(hip_ctx):
    """All 102 lifted graphs (2 base graphs x 51 lifting sizes) in one mixed plan: a random-LLR CB without CRC and a
    noisy codeword with CRC24B early termination per graph, each bit-exact vs the oracle."""
    cc = _cc()
    rng = np.random.default_rng(102)
    cases = []
    for bg in (1, 2):
        for Z in O.LIFTING_SIZES:
            L = O.BG_N_SHORT[bg] * Z
            cases.append((bg, Z, 5, O.NO_CRC, 0, random_llrs(rng, L, "mixed")))
            if O.BG_K[bg] * Z > 24 + 8:
                llr, _ = codeword_llrs(rng, bg, Z, 2.0, 1.1, crc=O.CRC24B)
                cases.append((bg, Z, 6, O.CRC24B, 0, llr))
    specs, out, res = _run_plan(hip_ctx, cc, cases)
    _check_against_oracle(cc, specs, cases, out, res)


# ldpc_spec.h LDPC_SPEC_GRAPHS: every (BG, Z) -- the core graphs (also bodies of the mixed kernel), the mid and the
# small lifting sizes
SPEC_GRAPHS = [(bg, z) for bg in (1, 2) for z in sorted(O.LIFTING_SIZES, reverse=True)]


@pytest.mark.parametrize("bg,Z", SPEC_GRAPHS)
def test_specialised_graph_batch(hip_ctx, bg, Z):
    """Each graph with a specialised kernel (ldpc_spec.h LDPC_SPEC_GRAPHS) as its own launch group (the specialised
    kernel's own launch, not the mixed one): random +-10 and 'mixed' (saturated, +-127) LLRs at full and shortened
    lengths (adaptive layer count, ldpc_decoder_impl.cpp:103-114), trailing zeros, filler bits, and noisy codewords
    with CRC16 / CRC24B early stop; 20 CBs, bit-exact vs the oracle."""
    cc = _cc()
    assert cc.specialised(bg, Z) == 1
    rng = np.random.default_rng(9000 + 10 * Z + bg)
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    cases = []
    for length in _create_range((K + 2) * Z, Ns * Z, 4) + [(K + 2) * Z + 1, Ns * Z - 3]:
        cases.append((bg, Z, 3, O.NO_CRC, 0, random_llrs(rng, length, "pm10")))
        cases.append((bg, Z, 2, O.NO_CRC, 0, random_llrs(rng, length, "mixed")))
    llr = random_llrs(rng, Ns * Z, "mixed")
    llr[-(7 * Z + 5):] = 0
    cases.append((bg, Z, 4, O.NO_CRC, 0, llr))
    # CRC and filler cases where the message holds them (tiny lifting sizes: K * Z down to 20 bits)
    for crc in (O.CRC16, O.CRC24B):
        if K * Z > 24 + 8:
            for snr in (1.6, 2.5):
                cw, _ = codeword_llrs(rng, bg, Z, snr, 1.0, crc=crc)
                cases.append((bg, Z, 8, crc, 0, cw))
    F = Z // 2 + 8
    if K * Z - F > 24 + 8:
        cw, _ = codeword_llrs(rng, bg, Z, 2.0, 1.0, F=F, crc=O.CRC24B)
        cases.append((bg, Z, 8, O.CRC24B, F, cw))
    specs, out, res = _run_plan(hip_ctx, cc, cases)
    _check_against_oracle(cc, specs, cases, out, res)


def test_specialised_graphs_full_batches(hip_ctx):
    """128 max-length CBs of every specialised graph in one plan (groups launched one after another on forked streams,
    all CUs busy; BG2 Z=256 runs two workgroups per CU): batch results equal per-CB oracle results on a sample."""
    import torch
    cc = _cc()
    from srsran_projectvtlmo_amd import _lib
    ctx = _flag_ctx(_lib.LAUNCH_NO_MIXED)
    try:
        for bg, Z in SPEC_GRAPHS:
            n = 128
            specs, ls, os_ = cc.uniform_batch_specs(n, bg, Z, 6)
            rng = np.random.default_rng(7 * Z + bg)
            h = (rng.integers(0, 2, (n, ls)) * 20 - 10).astype(np.int8)
            d_llr = torch.from_numpy(h.reshape(-1)).cuda()
            d_out = torch.zeros(n * os_, dtype=torch.uint8, device="cuda")
            plan = cc.DecodePlan(ctx, specs)
            plan.launch(d_llr.data_ptr(), d_out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            plan.close()
            out = d_out.cpu().numpy().reshape(n, os_)
            for i in (0, 1, 63, 127):
                ref, _ = O.ldpc_decode(bg, Z, h[i, :O.BG_N_SHORT[bg] * Z], 6)
                np.testing.assert_array_equal(out[i, :ref.size], ref, err_msg=f"BG{bg} Z={Z} cb {i}")
    finally:
        ctx.close()


def _flag_ctx(flags):
    from srsran_projectvtlmo_amd import _lib
    return _lib.Context(0, max_queue_cbs=256, nof_harq_slots=0, launch_flags=flags)


def test_every_lifted_graph_per_group_launches():
    """test_every_lifted_graph's plan (102 launch groups) with one launch per group on forked streams instead of the
    single mixed launch it gets by default (launch flag LDPC_HIP_LAUNCH_NO_MIXED): the same bit-exact results."""
    from srsran_projectvtlmo_amd import _lib
    ctx = _flag_ctx(_lib.LAUNCH_NO_MIXED)
    try:
        test_every_lifted_graph(ctx)
    finally:
        ctx.close()


def test_every_lifted_graph_generic_kernel():
    """test_every_lifted_graph with every graph on the generic kernel (launch flag LDPC_HIP_LAUNCH_NO_SPEC): the
    specialised schedules and the generic one give the same bit-exact results."""
    from srsran_projectvtlmo_amd import _lib
    ctx = _flag_ctx(_lib.LAUNCH_NO_SPEC)
    try:
        test_every_lifted_graph(ctx)
    finally:
        ctx.close()


_UNALIGNED = {}


def _unaligned_cases():
    """test_prologue_load_paths' codeblocks and their oracle results, built once for both bodies."""
    if not _UNALIGNED:
        rng = np.random.default_rng(316)
        kinds = []
        # BG1 Z=384 at full length (2Z and L multiples of 16); BG2 Z=36 (2Z = 72); BG1 Z=7 (odd: 2-byte LDS writes);
        # BG2 Z=208 shortened to a length that is no multiple of 16. CRC early stop on two of them, none on the others.
        kinds.append((1, 384, 4, O.NO_CRC, random_llrs(rng, O.BG_N_SHORT[1] * 384, "mixed")))
        kinds.append((2, 36, 3, O.NO_CRC, random_llrs(rng, O.BG_N_SHORT[2] * 36, "mixed")))
        kinds.append((1, 7, 4, O.CRC16, codeword_llrs(rng, 1, 7, 2.0, 0.9, crc=O.CRC16)[0]))
        kinds.append((2, 208, 4, O.CRC24B, codeword_llrs(rng, 2, 208, 2.0, 1.25, crc=O.CRC24B)[0][:50 * 208 - 5]))
        assert (2 * 36) % 16 != 0 and kinds[0][4].size % 16 == 0 and kinds[3][4].size % 16 != 0
        cases, skew = [], []
        for (bg, Z, it, crc, llr) in kinds:  # each codeblock at an offset = 0 and at an offset = 3 (mod 16)
            for sk in (0, 3):
                cases.append((bg, Z, it, crc, 0, llr))
                skew.append(sk)
        _UNALIGNED["cases"], _UNALIGNED["skew"] = cases, skew
        _UNALIGNED["expect"] = [O.ldpc_decode(bg, Z, llr, it, crc, F) for (bg, Z, it, crc, F, llr) in cases]
    return _UNALIGNED["cases"], _UNALIGNED["skew"], _UNALIGNED["expect"]


@pytest.mark.parametrize("body", ["specialised", "generic"])
def test_prologue_load_paths(body):
    """The prologue's three LLR load paths in both decoder bodies: codeblocks whose LLRs start at a multiple of 16 bytes
    (16-byte loads stored whole when 2Z and the length are multiples of 16, else through 4- or 2-byte LDS writes with a
    byte-wise tail) and 3 bytes after one (byte-wise loads). One plan per body: every graph on its specialised kernel
    (one launch per group, LDPC_HIP_LAUNCH_NO_MIXED) or on the generic kernel (LDPC_HIP_LAUNCH_NO_SPEC). Message, CRC
    flag and iteration count equal the oracle's."""
    from srsran_projectvtlmo_amd import _lib
    cc = _cc()
    cases, skew, expect = _unaligned_cases()
    ctx = _flag_ctx(_lib.LAUNCH_NO_MIXED if body == "specialised" else _lib.LAUNCH_NO_SPEC)
    try:
        if body == "specialised":
            assert all(cc.specialised(c[0], c[1]) == 1 for c in cases)
        specs, out, res = _run_plan(ctx, cc, cases, llr_skew=skew)
    finally:
        ctx.close()
    assert sorted({s.llr_offset % 16 for s in specs}) == [0, 3]
    for i, (s, (bg, Z, it, crc, F, llr), (eo, er)) in enumerate(zip(specs, cases, expect)):
        nb = cc.message_bytes(bg, Z)
        np.testing.assert_array_equal(out[s.out_offset:s.out_offset + nb], eo, err_msg=f"cb {i} BG{bg} Z={Z}")
        assert (res[i, 0] == 1) == (er is not None), f"cb {i} BG{bg} Z={Z}"
        # without a CRC pass the decoder runs every iteration (ldpc_decoder_impl.cpp:116-146)
        assert res[i, 1] == (er if er is not None else it), f"cb {i} BG{bg} Z={Z}"


def test_narrow_schedule_every_graph():
    """The narrow step schedule (at most 8 waves per workgroup, so two CBs share a CU; chosen automatically for groups
    of more CBs than CUs, e.g. C3) forced on every graph that has one (launch flag LDPC_HIP_LAUNCH_NARROW_ALWAYS):
    bit-exact vs the oracle, like the wide schedule -- both are the layer-serial order of
    ldpc_decoder_impl.cpp:116-123."""
    from srsran_projectvtlmo_amd import _lib
    # NO_SPEC too: graphs with a specialised kernel would otherwise run it instead of their narrow schedule
    hip_ctx = _flag_ctx(_lib.LAUNCH_NARROW_ALWAYS | _lib.LAUNCH_NO_MIXED | _lib.LAUNCH_NO_SPEC)
    cc = _cc()
    rng = np.random.default_rng(8)
    cases = []
    for bg in (1, 2):
        for Z in O.LIFTING_SIZES:
            L = O.BG_N_SHORT[bg] * Z
            cases.append((bg, Z, 4, O.NO_CRC, 0, random_llrs(rng, L, "mixed")))
            if O.BG_K[bg] * Z > 24 + 8:
                llr, _ = codeword_llrs(rng, bg, Z, 2.0, 1.1, crc=O.CRC24B)
                cases.append((bg, Z, 5, O.CRC24B, 0, llr))
    specs, out, res = _run_plan(hip_ctx, cc, cases)
    _check_against_oracle(cc, specs, cases, out, res)
    hip_ctx.close()


def test_c3_batch_1024_early_stop(hip_ctx):
    """C3 (BG2 Z=208, 1024 CBs, 10 iterations, CRC24B early termination) with the SURVEY §8d AWGN recipe: every CB
    bit-exact vs the oracle (message, CRC status, iteration count)."""
    cc = _cc()
    rng = np.random.default_rng(2)
    cases = []
    for _ in range(1024):
        llr, _ = codeword_llrs(rng, 2, 208, 2.0, 1.0, crc=O.CRC24B)
        cases.append((2, 208, 10, O.CRC24B, 0, llr))
    specs, out, res = _run_plan(hip_ctx, cc, cases)
    _check_against_oracle(cc, specs, cases, out, res)
    assert res[:, 0].sum() > 900      # at this SNR nearly every CB converges
