"""GPU parity of the specialised multi-wave decoder (sp::dec) with the extension edges of its odd-degree rows kept in
registers (ldpc_spec.h, ext_reg_edge): one codeblock per case through the C ABI against oracle.ldpc_decode on the
packed message, the CRC status and the iteration count.

Graphs: the smallest ones that run sp::dec (BG1 and BG2 at Z = 72, two waves per row), two with a half-filled last
wave (BG1 Z = 160, BG2 Z = 144, three waves per row) and BG1 Z = 384. Lengths: full, (K + 2) Z + 1 and one that leaves
10 layers (the partial-iteration loop). 1, 2 and 8 iterations. Vectors: mixed random LLRs and directed ones that drive
the promotion sum of the extension edges into saturation at the first or a later visit, with +127 fillers at the end of
the message. One early-stop case, one through the fused dematcher and one through the work queue."""
import numpy as np
import pytest

import oracle as O
from tests.vectors import codeword_llrs, random_llrs

pytestmark = pytest.mark.gpu

GRAPHS = [(1, 72), (2, 72), (1, 160), (2, 144), (1, 384)]
FILLERS = 24


@pytest.fixture(scope="module")
def launch_dec():
    """A decoder on the kernel-launch route (no work queue)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    ctx = _lib.Context(0, launch_flags=_lib.LAUNCH_NO_DWQ)
    yield cc, cc.ldpc_decoder_hip(ctx)
    ctx.close()


def _cfg(cc, bg, Z, iters, F):
    cfg = cc.configuration()
    cfg.block_conf.tb_common.base_graph = bg
    cfg.block_conf.tb_common.lifting_size = Z
    cfg.block_conf.cb_specific.nof_filler_bits = F
    cfg.algorithm_conf.max_iterations = iters
    return cfg


def _lengths(bg, Z):
    K, Ns = O.BG_K[bg], O.BG_N_SHORT[bg]
    return [Ns * Z, (K + 2) * Z + 1, (K + 8) * Z]  # 10 layers with the last: K + 8 columns + the 2 punctured ones


def _vectors(rng, bg, Z, L):
    """name -> int8 LLRs of length L (LLR i is codeword position i + 2 Z). The last FILLERS message positions are
    fillers (+127)."""
    K = O.BG_K[bg]
    col = (np.arange(L) + 2 * Z) // Z
    ext = col >= K + 4
    v = {"mixed": random_llrs(rng, L, "mixed")}
    v["all+100"] = np.full(L, 100, np.int8)
    v["info+100_ext+50"] = np.where(ext, 50, 100).astype(np.int8)
    v["info+30_ext+60"] = np.where(ext, 60, 30).astype(np.int8)  # no overflow at the first visit, one later
    stripes = np.array([120, -120, 127, -127, 0], np.int8)
    s = random_llrs(rng, L, "uniform")
    s[ext] = stripes[(col[ext] + np.arange(L)[ext]) % 5]
    v["ext_stripes"] = s
    s = (rng.integers(0, 2, L) * 2 - 1) * rng.integers(1, 40, L)  # small magnitudes: overflow at later visits
    s[ext] = (np.where(rng.integers(0, 2, L) == 1, -1, 1) * rng.integers(40, 121, L))[ext]
    v["small_info_large_ext"] = s.astype(np.int8)
    for a in v.values():
        a[K * Z - FILLERS - 2 * Z:K * Z - 2 * Z] = 127
    return v


@pytest.mark.parametrize("bg,Z", GRAPHS)
def test_ext_edges_bit_exact(launch_dec, bg, Z):
    cc, dec = launch_dec
    rng = np.random.default_rng(4200 + 10 * Z + bg)
    nb = (O.BG_K[bg] * Z + 7) // 8
    bad = []
    for L in _lengths(bg, Z):
        for name, llr in _vectors(rng, bg, Z, L).items():
            for iters in (1, 2, 8):
                out = np.full(nb, 0xA5, np.uint8)
                got = dec.decode(out, llr, None, _cfg(cc, bg, Z, iters, FILLERS))
                ref, ref_it = O.ldpc_decode(bg, Z, llr, iters, O.NO_CRC, FILLERS)
                if got != ref_it or not np.array_equal(out, ref):
                    bad.append((L, name, iters, int(np.count_nonzero(np.unpackbits(out ^ ref)))))
    assert not bad, f"BG{bg} Z={Z}: (length, vector, iterations, differing bits) {bad}"


@pytest.mark.parametrize("bg,Z,noise", [(1, 160, 1.6), (2, 144, 2.0), (1, 384, 1.6)])
def test_ext_edges_early_stop(launch_dec, bg, Z, noise):
    """CRC24B early termination: a codeword plus noise (enough of it for three iterations), fillers at +127; the
    iteration count must match."""
    cc, dec = launch_dec
    rng = np.random.default_rng(77 + Z)
    llr, _msg = codeword_llrs(rng, bg, Z, 2.0, noise, F=FILLERS, crc=O.CRC24B)
    out = np.full((O.BG_K[bg] * Z + 7) // 8, 0xA5, np.uint8)
    got = dec.decode(out, llr, cc.crc_calculator("CRC24B"), _cfg(cc, bg, Z, 8, FILLERS))
    ref, ref_it = O.ldpc_decode(bg, Z, llr, 8, O.CRC24B, FILLERS)
    assert ref_it is not None and ref_it > 1  # the case does stop early, after more than one iteration
    assert got == ref_it
    np.testing.assert_array_equal(out, ref)


def test_ext_edges_work_queue():
    """The same decoder body on the device work queue (the default route of a one-codeblock call)."""
    from srsran_projectvtlmo_amd import _lib
    from srsran_projectvtlmo_amd import channel_coding as cc
    ctx = _lib.Context(0)
    try:
        dec = cc.ldpc_decoder_hip(ctx)
        for bg, Z in ((1, 384), (2, 72)):
            rng = np.random.default_rng(900 + Z)
            L = O.BG_N_SHORT[bg] * Z
            for name, llr in _vectors(rng, bg, Z, L).items():
                out = np.full((O.BG_K[bg] * Z + 7) // 8, 0xA5, np.uint8)
                got = dec.decode(out, llr, None, _cfg(cc, bg, Z, 8, FILLERS))
                ref, ref_it = O.ldpc_decode(bg, Z, llr, 8, O.NO_CRC, FILLERS)
                assert got == ref_it and np.array_equal(out, ref), (bg, Z, name)
    finally:
        ctx.close()


def test_ext_edges_fused_dematch(hip_ctx):
    """A first transmission at rv 0 through ldpc_hip_dematch_decode_launch (the dematcher fused into the decode
    kernel): one five-codeblock BG1 Z = 384 transport block, per-CB CRC flags and iteration counts, TB bytes."""
    import torch

    from srsran_projectvtlmo_amd import pusch
    from tests.tb_chain import SwFlow, TransportBlock
    rng = np.random.default_rng(55)
    tb = TransportBlock(rng, 40000, 1, 14000, "QAM256", 4)
    assert tb.bg == 1 and tb.Z == 384
    spec = pusch.tb_slot_spec(tb.tbs, tb.bg, tb.Z, tb.F, [m["rm_length"] for m in tb.metas], tb.Qm, 0, True, 0, 8, True)
    pipe = pusch.SlotPipeline(hip_ctx, [spec], fuse_dematch=True)
    flow = SwFlow(tb, nof_iters=8, early_stop=True)
    llr = tb.llrs(rng, 0, 2.0, 0.7)
    pipe.upload([llr])
    pipe.launch(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, cbres = pipe.results()
    ok, _bits = flow.transmission(llr, 0, True)
    for r in range(tb.C):
        assert bool(cbres[r, 0]) == flow.crc_ok[r], f"cb {r} crc"
        if flow.crc_ok[r]:
            assert cbres[r, 1] == flow.iters_used[r], f"cb {r} iterations"
    tb_bytes, g_ok, _written = got[0]
    assert g_ok == ok
    if ok:
        assert np.array_equal(np.unpackbits(tb_bytes)[:tb.tbs], tb.data)
