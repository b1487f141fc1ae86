"""GPU tests whose expected values are what the compiled reference itself wrote (tests/golden/ref_*.npz, recorded by
tests/golden/make_reference_fixtures.py). The oracle is not called here: a misreading shared by the oracle and a kernel
fails these tests. Inputs are regenerated from the recorded seeds and checked against the recorded digests
(tests/ref_cases.load_fixture); comparisons are exact (tests/ref_cases.compare)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import ref_cases as C
from tests import scrambling_ref as R

pytestmark = pytest.mark.gpu

HIP_CRC = {-1: -1, 3: 0, 1: 1, 0: 2}   # oracle / crc_generator_poly numbering -> hw_dec_cb_crc_type
CRC_NAME = {3: "CRC16", 1: "CRC24B", 0: "CRC24A"}
MOD_NAME = {1: "BPSK", 2: "QPSK", 4: "QAM16", 6: "QAM64", 8: "QAM256"}


@functools.lru_cache(maxsize=None)
def _fixture(op):
    return C.load_fixture(op)


def _assert_equal(op, cases, got, want):
    bad = [(c, names) for c, g, w in zip(cases, got, want) for names in [C.compare(g, w)] if names]
    assert cases and not bad, f"{op}: {len(bad)} of {len(cases)} differ from the reference, first: {bad[:4]}"


def _flag_ctx(flags, harq=0):
    from srsran_projectvtlmo_amd import _lib
    return _lib.Context(0, max_queue_cbs=256, nof_harq_slots=harq, launch_flags=flags)


def _al(n):
    return (n + 15) // 16 * 16


# ---- decoder ----------------------------------------------------------------------------------------------------------
def _decode_plan(ctx, cases, inputs):
    """One DecodePlan over the cases, in their order; returns run_decode-shaped results."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    specs = []
    lo = oo = 0
    for c, llr in zip(cases, inputs):
        mode = cc.CRC_MODE_NONE if c["crc"] < 0 else cc.CRC_MODE_EARLY_STOP
        specs.append(cc.cb_decode_spec(c["bg"], c["Z"], llr.size, c["iters"], mode, HIP_CRC[c["crc"]], c["F"], c["sf"],
                                       lo, oo))
        lo += _al(llr.size)
        oo += _al(cc.message_bytes(c["bg"], c["Z"]))
    h = np.zeros(lo, np.int8)
    for s, llr in zip(specs, inputs):
        h[s.llr_offset:s.llr_offset + llr.size] = llr
    d_llr = torch.from_numpy(h).cuda()
    d_out = torch.zeros(oo, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(len(specs) * 4, dtype=torch.uint8, device="cuda")
    plan = cc.DecodePlan(ctx, specs)
    try:
        plan.launch(d_llr.data_ptr(), d_out.data_ptr(), d_res.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        plan.close()
    out, res = d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 4)
    return [_decode_result(out[s.out_offset:s.out_offset + cc.message_bytes(s.base_graph, s.lifting_size)],
                           bool(r[0]), int(r[1])) for s, r in zip(specs, res)]


def _decode_result(msg, ok, iters):
    return {"msg": msg, "ok": np.array([ok], np.uint8), "iters": np.array([iters if ok else 0], np.uint8)}


ROUTES = {"default": 0, "no_mixed": 0x2, "no_spec": 0x1, "narrow": 0x4 | 0x2 | 0x1}


def _route_ctx(route, hip_ctx):
    from srsran_projectvtlmo_amd import _lib
    assert (_lib.LAUNCH_NO_SPEC, _lib.LAUNCH_NO_MIXED, _lib.LAUNCH_NARROW_ALWAYS) == (0x1, 0x2, 0x4)
    return hip_ctx if route == "default" else _flag_ctx(ROUTES[route])


@pytest.mark.parametrize("route", list(ROUTES))
def test_decode_every_graph_default_sf(hip_ctx, route):
    """Every (BG, Z), a full-length and a shortened CB: specialised kernels in the mixed launch, one launch per
    group, the generic kernel, and the narrow schedule."""
    cases, outs, inputs = _fixture("decode")
    ctx = _route_ctx(route, hip_ctx)
    try:
        _assert_equal(f"decode ({route})", cases, _decode_plan(ctx, cases, inputs), outs)
    finally:
        if ctx is not hip_ctx:
            ctx.close()


@pytest.mark.parametrize("sf", C.SFS_FIXTURE)
def test_decode_every_graph_one_scaling_factor(hip_ctx, sf):
    """All 102 graphs at one non-default scaling factor in one plan (the SF08 = false kernel on BG1's degree-19 rows,
    split rows, one-wave and multi-wave graphs)."""
    cases, outs, inputs = _fixture("decode_sf")
    pick = [i for i, c in enumerate(cases) if c["sf"] == sf]
    assert len(pick) == len(C.GRAPHS)
    _assert_equal(f"decode sf={sf}", [cases[i] for i in pick],
                  _decode_plan(hip_ctx, [cases[i] for i in pick], [inputs[i] for i in pick]), [outs[i] for i in pick])


def test_decode_plan_mixing_scaling_factors(hip_ctx):
    """One plan with the four non-default factors and sf = 0.8 CBs of the same graphs interleaved in input order: the
    planner groups by (slot, sf08) and never launches a group that mixes them; results come back in input order."""
    c_sf, o_sf, i_sf = _fixture("decode_sf")
    c_08, o_08, i_08 = _fixture("decode")
    cases, outs, inputs = [], [], []
    for g in range(len(C.GRAPHS)):
        for k in range(4):
            cases.append(c_sf[4 * g + k]), outs.append(o_sf[4 * g + k]), inputs.append(i_sf[4 * g + k])
            if k % 2 == 0:
                j = 2 * g + k // 2
                cases.append(c_08[j]), outs.append(o_08[j]), inputs.append(i_08[j])
    assert {c["sf"] for c in cases} == set(C.SFS_FIXTURE) | {0.8}
    _assert_equal("decode mixed sf", cases, _decode_plan(hip_ctx, cases, inputs), outs)


def test_decode_narrow_route_half_scaling(hip_ctx):
    """sf = 0.5 (every scaled magnitude an exact rounding tie or an integer) on the narrow schedule."""
    cases, outs, inputs = _fixture("decode_sf")
    pick = [i for i, c in enumerate(cases) if c["sf"] == 0.5]
    ctx = _flag_ctx(ROUTES["narrow"])
    try:
        _assert_equal("decode narrow sf=0.5", [cases[i] for i in pick],
                      _decode_plan(ctx, [cases[i] for i in pick], [inputs[i] for i in pick]), [outs[i] for i in pick])
    finally:
        ctx.close()


@pytest.mark.parametrize("dwq", [True, False])
def test_decode_single_cbs_sync_adapter(dwq):
    """ldpc_decoder_hip (ldpc_hip_decode_sync picks its path on scaling_factor != 0.8f): two graphs per scaling factor,
    the default one included, with the device work queue and with the launch path."""
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    c_sf, o_sf, i_sf = _fixture("decode_sf")
    c_08, o_08, i_08 = _fixture("decode")
    graphs = [(1, 384), (2, 52), (1, 36), (2, 208), (1, 7), (2, 384), (1, 104), (2, 15)]
    pick = []
    for k, sf in enumerate(C.SFS_FIXTURE):
        pick += [(c, o, i) for c, o, i in zip(c_sf, o_sf, i_sf)
                 if c["sf"] == sf and (c["bg"], c["Z"]) in graphs[2 * k:2 * k + 2]]
    pick += [(c, o, i) for c, o, i in zip(c_08, o_08, i_08) if (c["bg"], c["Z"]) in graphs[:2]]
    assert len(pick) == 12
    ctx = _flag_ctx(0 if dwq else _lib.LAUNCH_NO_DWQ)
    try:
        dec = cc.ldpc_decoder_hip(ctx)
        got = []
        for c, _, llr in pick:
            cfg = cc.configuration()
            cfg.block_conf.tb_common.base_graph, cfg.block_conf.tb_common.lifting_size = c["bg"], c["Z"]
            cfg.block_conf.cb_specific.nof_filler_bits = c["F"]
            cfg.algorithm_conf.max_iterations, cfg.algorithm_conf.scaling_factor = c["iters"], c["sf"]
            out = np.zeros(cc.message_bytes(c["bg"], c["Z"]), np.uint8)
            it = dec.decode(out, llr, None, cfg)
            got.append(_decode_result(out, it is not None, it or 0))
        _assert_equal("decode sync", [p[0] for p in pick], got, [p[1] for p in pick])
    finally:
        ctx.close()


def test_early_stop(hip_ctx):
    """The stored noisy codewords, 10 iterations, CRC16 / CRC24A / CRC24B and fillers: CRC flag, iteration count and
    message (the last iteration's hard bits when the CRC fails) as the reference gave them; then CB by CB through the
    sync adapter."""
    from srsran_projectvtlmo_amd import channel_coding as cc
    cases, outs, inputs = _fixture("early_stop")
    assert any(0 < int(o["iters"][0]) < 10 for o in outs) and any(int(o["ok"][0]) == 0 for o in outs)
    _assert_equal("early stop", cases, _decode_plan(hip_ctx, cases, inputs), outs)
    dec = cc.ldpc_decoder_hip(hip_ctx)
    got = []
    for c, llr in zip(cases, inputs):
        cfg = cc.configuration()
        cfg.block_conf.tb_common.base_graph, cfg.block_conf.tb_common.lifting_size = c["bg"], c["Z"]
        cfg.block_conf.cb_specific.nof_filler_bits = c["F"]
        cfg.algorithm_conf.max_iterations = c["iters"]
        out = np.zeros(cc.message_bytes(c["bg"], c["Z"]), np.uint8)
        it = dec.decode(out, llr, cc.crc_calculator(CRC_NAME[c["crc"]]), cfg)
        got.append(_decode_result(out, it is not None, it or 0))
    _assert_equal("early stop sync", cases, got, outs)


# ---- rate dematcher ---------------------------------------------------------------------------------------------------
def _dm_descs(cases, new_data, rvs=None):
    from srsran_projectvtlmo_amd import _lib
    dm = (_lib.DematchDesc * len(cases))()
    for k, (d, c) in enumerate(zip(dm, cases)):
        d.modulation_order, d.rv, d.new_data = c["Qm"], c["rv"] if rvs is None else rvs, int(new_data)
        d.cb_length, d.rm_length = 50 * c["Z"] if c["bg"] == 2 else 66 * c["Z"], c["E"]
        d.Nref, d.nof_filler_bits = c.get("Nref", 0), c["F"]
    return dm


def test_rate_dematch_sync_adapter(hip_ctx):
    """ldpc_rate_dematcher_hip on every recorded case: a new-data pass over a stale buffer, a combining pass into it,
    and a combining pass into the stale buffer itself; buffers and inputs hold +-127 of both signs and +-120."""
    from srsran_projectvtlmo_amd import channel_coding as cc
    cases, outs, inputs = _fixture("dematch")
    dm = cc.ldpc_rate_dematcher_hip(hip_ctx)
    got = []
    for c, (start, tx1, tx2) in zip(cases, inputs):
        meta = cc.codeblock_metadata()
        meta.tb_common.rv, meta.tb_common.mod, meta.tb_common.Nref = c["rv"], MOD_NAME[c["Qm"]], c["Nref"]
        meta.cb_specific.nof_filler_bits = c["F"]
        a = start.copy()
        dm.rate_dematch(a, tx1, True, meta)
        new = a.copy()
        dm.rate_dematch(a, tx2, False, meta)
        b = start.copy()
        dm.rate_dematch(b, tx1, False, meta)
        got.append({"soft_new": new, "soft_comb": a, "soft_comb0": b})
    _assert_equal("rate dematch sync", cases, got, outs)


def _dematch_launch(hip_ctx, cases, txs, d_soft, soft_off, new_data, shift, scr=None):
    """All cases in one ldpc_hip_rate_dematch_launch (or _scr_launch), CB k's input at a device offset = shift mod 16."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    n = len(cases)
    offs, pos = [], 0
    for t in txs:
        offs.append(pos + shift)
        pos += _al(t.size) + 32
    h = np.zeros(pos, np.int8)
    for o, t in zip(offs, txs):
        h[o:o + t.size] = t
    d_llr = torch.from_numpy(h).cuda()
    u64 = ctypes.c_uint64 * n
    dm = _dm_descs(cases, new_data)
    if scr is None:
        rc = hip_ctx.lib.ldpc_hip_rate_dematch_launch(hip_ctx.handle, n, dm, d_llr.data_ptr(), u64(*offs),
                                                      d_soft.data_ptr(), u64(*soft_off), _lib.stream_arg(0))
    else:
        rc = hip_ctx.lib.ldpc_hip_rate_dematch_scr_launch(hip_ctx.handle, n, dm, d_llr.data_ptr(), u64(*offs), None,
                                                          None, None, scr, d_soft.data_ptr(), u64(*soft_off),
                                                          _lib.stream_arg(0))
    assert rc == 0, hip_ctx.lib.ldpc_hip_last_error(hip_ctx.handle)
    torch.cuda.synchronize()


def _soft_layout(cases, inputs):
    import torch
    soft_off, pos = [], 0
    for start, _, _ in inputs:
        soft_off.append(pos)
        pos += _al(start.size)
    h = np.zeros(pos, np.int8)
    for o, (start, _, _) in zip(soft_off, inputs):
        h[o:o + start.size] = start
    return torch.from_numpy(h).cuda(), soft_off


def test_rate_dematch_launch_unaligned_input(hip_ctx):
    """ldpc_hip_rate_dematch_launch, every case in one launch, inputs at device offsets 3 and 5 mod 16 (the byte-load
    path; E around the LDS staging limit among them): the new-data pass, then the combining pass."""
    cases, outs, inputs = _fixture("dematch")
    d_soft, soft_off = _soft_layout(cases, inputs)
    _dematch_launch(hip_ctx, cases, [i[1] for i in inputs], d_soft, soft_off, True, 3)
    new = d_soft.cpu().numpy()
    _dematch_launch(hip_ctx, cases, [i[2] for i in inputs], d_soft, soft_off, False, 5)
    comb = d_soft.cpu().numpy()
    got = [{"soft_new": new[o:o + i[0].size], "soft_comb": comb[o:o + i[0].size]} for o, i in zip(soft_off, inputs)]
    want = [{k: o[k] for k in ("soft_new", "soft_comb")} for o in outs]
    _assert_equal("rate dematch launch", cases, got, want)


def test_rate_dematch_scrambled_input(hip_ctx):
    """ldpc_hip_rate_dematch_scr_launch: the recorded inputs scrambled with the descrambler fixture's sequences (the sign
    flips are their own inverse), descrambled inside the dematcher; every case that fits the LDS staging."""
    from srsran_projectvtlmo_amd import sequence_generators as sg
    cases, outs, inputs = _fixture("dematch")
    seqs = [(c["c_init"], c["offset"]) for c in _fixture("descramble")[0]]
    pick = [k for k, c in enumerate(cases) if c["E"] <= C.DM_STAGE]
    assert len(pick) >= 10
    cs, ins = [cases[k] for k in pick], [inputs[k] for k in pick]
    use = [seqs[k % len(seqs)] for k in range(len(cs))]
    d_soft, soft_off = _soft_layout(cs, ins)
    scr = sg.scramble_descriptors(use)
    for name, idx, new_data, shift in (("soft_new", 1, True, 0), ("soft_comb", 2, False, 7)):
        txs = [R.descramble(i[idx], ci, off) for i, (ci, off) in zip(ins, use)]
        _dematch_launch(hip_ctx, cs, txs, d_soft, soft_off, new_data, shift, scr)
        soft = d_soft.cpu().numpy()
        _assert_equal(f"scrambled dematch {name}", cs, [{name: soft[o:o + i[0].size]} for o, i in zip(soft_off, ins)],
                      [{name: outs[k][name]} for k in pick])


def test_dematch_decode_chains(hip_ctx_harq):
    """rv 0 with new data, then rv 2 combined into the same device soft buffers, the dematcher fused into the decode
    kernels (ldpc_hip_dematch_decode_launch): both stages' soft buffers, messages, CRC flags and iteration counts."""
    import torch
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    ctx = hip_ctx_harq
    cases, outs, inputs = _fixture("chain")
    n = len(cases)
    specs, so, oo = [], 0, 0
    for c in cases:
        N = (66 if c["bg"] == 1 else 50) * c["Z"]
        specs.append(cc.cb_decode_spec(c["bg"], c["Z"], N, c["iters"], cc.CRC_MODE_EARLY_STOP, HIP_CRC[c["crc"]],
                                       c["F"], 0.8, so, oo))
        so += _al(N)
        oo += _al(cc.message_bytes(c["bg"], c["Z"]))
    d_soft = torch.zeros(so, dtype=torch.int8, device="cuda")
    d_out = torch.zeros(oo, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    plan = cc.DecodePlan(ctx, specs)
    got = [dict() for _ in cases]
    try:
        for k, rv in enumerate((0, 2)):
            offs, pos = [], 0
            for i in inputs:
                offs.append(pos + (3 if k else 0))
                pos += _al(i[k].size) + 16
            h = np.zeros(pos, np.int8)
            for o, i in zip(offs, inputs):
                h[o:o + i[k].size] = i[k]
            d_llr = torch.from_numpy(h).cuda()
            rc = ctx.lib.ldpc_hip_dematch_decode_launch(plan.handle, _dm_descs(cases, k == 0, rv), d_llr.data_ptr(),
                                                        (ctypes.c_uint64 * n)(*offs), None, None, None,
                                                        d_soft.data_ptr(), d_out.data_ptr(), d_res.data_ptr(),
                                                        _lib.stream_arg(0))
            assert rc == 0, ctx.lib.ldpc_hip_last_error(ctx.handle)
            torch.cuda.synchronize()
            soft, out, res = d_soft.cpu().numpy(), d_out.cpu().numpy(), d_res.cpu().numpy().reshape(-1, 4)
            for g, s, r in zip(got, specs, res):
                g[f"soft{k}"] = soft[s.llr_offset:s.llr_offset + s.llr_length]
                g[f"msg{k}"] = out[s.out_offset:s.out_offset + cc.message_bytes(s.base_graph, s.lifting_size)]
                g[f"iters{k}"] = np.array([int(r[1]) if r[0] else 0], np.uint8)
    finally:
        plan.close()
    _assert_equal("dematch -> decode chain", cases, got, outs)


# ---- demodulator and descrambler ------------------------------------------------------------------------------------
def test_demodulator(hip_ctx):
    """257 symbols per scheme (the 16-QAM entry is the input that exposed the +-24 quantisation range) and the special
    values (NaN, infinities, bad noise variances: the reference as compiled on x86-64)."""
    from srsran_projectvtlmo_amd import channel_modulation as cm
    cases, outs, inputs = _fixture("demod")
    assert any(c.get("name") == "qam16_range_limit_20" for c in cases)
    dm = cm.create_channel_modulation_hip_factory(hip_ctx).create_demodulation_mapper()
    got = []
    for c, (sym, nv) in zip(cases, inputs):
        out = np.zeros(sym.size * cm.get_bits_per_symbol(c["mod"]), np.int8)
        dm.demodulate_soft(out, sym, nv, c["mod"])
        got.append({"llr": out})
    _assert_equal("demodulate", cases, got, outs)


def test_descrambler(hip_ctx):
    """The generator object on LLRs and on packed bits: several c_init, lengths with and without a 32-bit tail, non-zero
    sequence offsets."""
    from srsran_projectvtlmo_amd import sequence_generators as sg
    cases, outs, inputs = _fixture("descramble")
    gen = sg.pseudo_random_generator_hip(hip_ctx)
    got = []
    for c, llr in zip(cases, inputs):
        gen.init(c["c_init"])
        gen.advance(c["offset"])
        a = gen.apply_xor(llr)
        gen.init(c["c_init"])
        gen.advance(c["offset"])
        bits = (llr.astype(np.int16) & 1).astype(np.uint8)
        got.append({"llr": a, "packed": gen.apply_xor(np.packbits(bits), c["n"])})
    _assert_equal("descramble", cases, got, outs)


# ---- encoder and rate matcher -----------------------------------------------------------------------------------------
def test_encoder_every_graph(hip_ctx):
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    cases, outs, inputs = _fixture("encode")
    specs, mo, co = [], 0, 0
    for c, msg in zip(cases, inputs):
        specs.append(cc.cb_encode_spec(c["bg"], c["Z"], c["L"], mo, co))
        mo += _al((msg.size + 7) // 8)
        co += _al((c["L"] + 7) // 8)
    h = np.zeros(mo, np.uint8)
    for s, msg in zip(specs, inputs):
        p = np.packbits(np.where(msg > 1, 0, msg).astype(np.uint8))
        h[s.msg_offset:s.msg_offset + p.size] = p
    d_msg = torch.from_numpy(h).cuda()
    d_cw = torch.zeros(co, dtype=torch.uint8, device="cuda")
    cc.encode_launch(hip_ctx, specs, d_msg.data_ptr(), d_cw.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cw = d_cw.cpu().numpy()
    got = [{"cw": np.packbits(np.unpackbits(cw[s.cw_offset:s.cw_offset + (s.cw_length + 7) // 8])[:s.cw_length])}
           for s in specs]
    _assert_equal("encode", cases, got, [{"cw": o["cw"]} for o in outs])


def test_rate_matcher(hip_ctx):
    """All RVs, Qm in {1, 2, 4, 6, 8}, limited and unlimited buffers, with and without fillers."""
    import torch
    from srsran_projectvtlmo_amd import channel_coding as cc
    cases, outs, inputs = _fixture("rate_match")
    specs, co, oo = [], 0, 0
    for c, cw in zip(cases, inputs):
        specs.append(cc.cb_rate_match_spec(cw.size, c["E"], c["Qm"], c["rv"], c["Nref"], c["F"], co, oo))
        co += _al((cw.size + 7) // 8)
        oo += _al((c["E"] + 7) // 8)
    h = np.zeros(co, np.uint8)
    for s, cw in zip(specs, inputs):
        p = np.packbits(np.where(cw > 1, 0, cw).astype(np.uint8))
        h[s.cw_offset:s.cw_offset + p.size] = p
    d_cw = torch.from_numpy(h).cuda()
    d_out = torch.zeros(oo, dtype=torch.uint8, device="cuda")
    cc.rate_match_launch(hip_ctx, specs, d_cw.data_ptr(), d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    got = [{"bits": np.packbits(np.unpackbits(out[s.out_offset:s.out_offset + (s.rm_length + 7) // 8])[:s.rm_length])}
           for s in specs]
    _assert_equal("rate match", cases, got, outs)
