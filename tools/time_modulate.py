"""GPU box: what scrambling and mapping rate-matched bits to symbols costs. Device events over
graph replays after warm-up, the variants alternating in one process, several rounds per variant, so the spread of
repeated identical measurements stands beside the differences.

Workload: the C4 slot's downlink mirror: UE0's 128 codeblocks BG1 Z=384 256-QAM (E = 9,728 / 9,760) and 23 one-codeblock
BG2 Z=36 QPSK TBs (E = 1,248), every codeword scrambled; the codeword bytes are random (neither the rate matcher nor the
mapper's time depends on them).

  mod_<fmt>     ldpc_hip_modulate_launch over the slot's rate-matched bits, scrambling on, one segment per codeblock;
                kernel time and GB/s of bits read plus symbols written
  mod_plain_<fmt>  the same launch with scrambling off: the same bytes read and written, without the sequence arithmetic
  fused_<fmt>   ldpc_hip_rate_match_modulate_launch
  three_<fmt>   the same result by three launches: ldpc_hip_rate_match_launch, ldpc_hip_scramble_bits_launch in place,
                ldpc_hip_modulate_launch without scrambling
  rate_match    ldpc_hip_rate_match_launch alone (the only variant a build of the parent commit has: LIB_SUFFIX names
                such a library, as in tools/batch_time_lib.py; '-' is the product library)

Each graph holds CHAIN repetitions of its variant; times are per repetition. Every variant has a context of its own: a
launch's descriptor table lives in a per-context device buffer that a captured kernel node only points to, so variants
sharing a context would replay with whichever table was uploaded last. After the rounds the mod_cf32 graph's symbols
are compared with an unscrambled mapping of the same bits (they must differ) and with a scrambled eager launch (equal).

usage: python tools/time_modulate.py LIB_SUFFIX|- [reps] [rounds]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from srsran_projectvtlmo_amd import _lib  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
if sys.argv[1] != "-":
    _lib.LIB_PATH = ROOT / "srsran_projectvtlmo_amd" / "lib" / f"libsrsran_ldpc_hip_{sys.argv[1]}.so"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
CHAIN = 10


def _time(fn, stream, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    for _ in range(reps):
        fn()
    ev[1].record(stream)
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3  # us


class bare_context:
    """A context on a library bound by hand: only the entry points the rate_match variant needs, so a build of the
    parent commit (which has no mapper) loads without the package's full binding."""

    def __init__(self, path, device=0):
        import ctypes
        P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
        L = ctypes.CDLL(str(path))
        for name, res, args in (("ldpc_hip_open", I, [I, ctypes.POINTER(_lib.Params), ctypes.POINTER(P)]),
                                ("ldpc_hip_close", I, [P]), ("ldpc_hip_last_error", ctypes.c_char_p, [P]),
                                ("ldpc_hip_rate_match_launch", I, [P, U32, ctypes.POINTER(_lib.RmDesc), P, P, P]),
                                ("ldpc_hip_capture_begin", I, [P, P]),
                                ("ldpc_hip_capture_end", I, [P, P, ctypes.POINTER(P)]),
                                ("ldpc_hip_graph_launch", I, [P, P]), ("ldpc_hip_graph_destroy", I, [P])):
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        self.lib, self.handle = L, P()
        params = _lib.Params(0, 0, 0, 0)
        if L.ldpc_hip_open(device, ctypes.byref(params), ctypes.byref(self.handle)) != 0:
            raise RuntimeError(f"ldpc_hip_open on {path} failed")

    def close(self):
        self.lib.ldpc_hip_close(self.handle)


def _ok(ctx, rc, what):
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {ctx.lib.ldpc_hip_last_error(ctx.handle)}")


def main():
    import ctypes

    import torch

    from srsran_projectvtlmo_amd import channel_coding as cc
    from srsran_projectvtlmo_amd import segmentation as S
    has_mod = hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "ldpc_hip_modulate_launch")
    new_ctx = (lambda: _lib.Context(0)) if has_mod else (lambda: bare_context(_lib.LIB_PATH))
    from srsran_projectvtlmo_amd import channel_modulation as cm
    from srsran_projectvtlmo_amd import sequence_generators as sg
    stream = torch.cuda.Stream()
    ues = [(1078248, 1, 250 * 156 * 4, 8, 4)] + [(256, 2, 156 * 4, 2, 4)] * 23
    rm, mods, plain, prs = [], [], [], []
    co = oo = so = 0
    for k, (tbs, bg, nsym, qm, layers) in enumerate(ues):
        metas = S.segment_rx(tbs, bg, nsym, qm, layers)
        m0, seq = metas[0], 0
        N = cc.BG_N_SHORT[bg] * m0.lifting_size
        c_init = ((0x4601 + k) << 15) + 17 * k
        for m in metas:
            E = m.rm_length
            rm.append(cc.cb_rate_match_spec(N, E, qm, 0, 0, m0.nof_filler_bits, co, oo))
            mods.append(cm.mod_segment(E // qm, qm, oo, so, True, c_init, seq))
            plain.append(cm.mod_segment(E // qm, qm, oo, so))
            prs.append(sg.prs_segment(E, c_init, seq, oo, oo))
            co += ((N + 7) // 8 + 15) // 16 * 16
            oo += ((E + 7) // 8 + 15) // 16 * 16
            so += (E // qm + 7) // 8 * 8
            seq += E
    nbits = sum(r.rm_length for r in rm)
    rm_arr = (_lib.RmDesc * len(rm))()
    for a, sp in zip(rm_arr, rm):
        a.cw_offset, a.out_offset, a.cb_length, a.rm_length = sp.cw_offset, sp.out_offset, sp.cb_length, sp.rm_length
        a.Nref, a.nof_filler_bits, a.modulation_order, a.rv = sp.Nref, sp.nof_filler_bits, sp.modulation_order, sp.rv
    d_cw = torch.randint(0, 256, (co,), dtype=torch.uint8, device="cuda")
    d_bits = torch.zeros(oo, dtype=torch.uint8, device="cuda")       # the rate matcher's and the three-launch path's
    d_in = torch.randint(0, 256, (oo,), dtype=torch.uint8, device="cuda")   # the stand-alone mapper's input
    d_sym = torch.zeros(so * 8, dtype=torch.uint8, device="cuda")
    s = stream.cuda_stream
    ctxs, variants = {}, {}

    def add(name, make):
        ctxs[name] = new_ctx()
        variants[name] = make(ctxs[name])

    add("rate_match", lambda c: lambda: _ok(c, c.lib.ldpc_hip_rate_match_launch(
        c.handle, len(rm), rm_arr, d_cw.data_ptr(), d_bits.data_ptr(), s), "rate_match_launch"))
    if has_mod:
        prs_arr, mod_arr, plain_arr = sg.prs_descriptors(prs), cm.mod_descriptors(mods), cm.mod_descriptors(plain)
        for name, fmt in (("cf32", _lib.SYM_CF32), ("ci8", _lib.SYM_CI8)):
            add(f"mod_{name}", lambda c, fmt=fmt: lambda: cm.modulate_launch(
                c, mod_arr, d_in.data_ptr(), d_sym.data_ptr(), fmt, s, n=len(mods)))
            add(f"mod_plain_{name}", lambda c, fmt=fmt: lambda: cm.modulate_launch(
                c, plain_arr, d_in.data_ptr(), d_sym.data_ptr(), fmt, s, n=len(plain)))
            add(f"fused_{name}", lambda c, fmt=fmt: lambda: cm.rate_match_modulate_launch(
                c, rm, mods, d_cw.data_ptr(), d_sym.data_ptr(), fmt, s))

            def three(c, fmt=fmt):
                def run():
                    cc.rate_match_launch(c, rm, d_cw.data_ptr(), d_bits.data_ptr(), s)
                    sg.scramble_bits_launch(c, prs_arr, d_bits.data_ptr(), d_bits.data_ptr(), s, n=len(prs))
                    cm.modulate_launch(c, plain_arr, d_bits.data_ptr(), d_sym.data_ptr(), fmt, s, n=len(plain))
                return run
            add(f"three_{name}", three)
    graphs = {}
    for name, fn in variants.items():
        c = ctxs[name]
        fn()                      # descriptors uploaded before the capture
        stream.synchronize()
        _ok(c, c.lib.ldpc_hip_capture_begin(c.handle, s), "capture_begin")
        for _ in range(CHAIN):
            fn()
        g = ctypes.c_void_p()
        _ok(c, c.lib.ldpc_hip_capture_end(c.handle, s, ctypes.byref(g)), "capture_end")
        graphs[name] = g
        _time(lambda: c.lib.ldpc_hip_graph_launch(g, s), stream, reps)  # warm-up
    times = {name: [] for name in graphs}
    for _ in range(rounds):       # alternate the variants
        for name, g in graphs.items():
            L = ctxs[name].lib
            times[name].append(round(_time(lambda: L.ldpc_hip_graph_launch(g, s), stream, reps) / CHAIN, 2))
    out = {"lib": _lib.LIB_PATH.name, "reps": reps, "rounds": rounds, "chain": CHAIN, "codeblocks": len(rm),
           "rate_matched_bits": nbits, "symbols": sum(m.nof_symbols for m in mods)}
    if has_mod:
        # what the timed mod_cf32 graph computes: the scrambled mapping, not the plain one
        ctxs["mod_cf32"].lib.ldpc_hip_graph_launch(graphs["mod_cf32"], s)
        stream.synchronize()
        replay = d_sym.clone()
        check = new_ctx()
        cm.modulate_launch(check, mod_arr, d_in.data_ptr(), d_sym.data_ptr(), _lib.SYM_CF32, s, n=len(mods))
        stream.synchronize()
        out["mod_cf32_replay_equals_scrambled_eager"] = bool(torch.equal(replay, d_sym))
        cm.modulate_launch(check, plain_arr, d_in.data_ptr(), d_sym.data_ptr(), _lib.SYM_CF32, s, n=len(plain))
        stream.synchronize()
        out["mod_cf32_replay_differs_from_unscrambled"] = not bool(torch.equal(replay, d_sym))
        check.close()
        if not (out["mod_cf32_replay_equals_scrambled_eager"] and out["mod_cf32_replay_differs_from_unscrambled"]):
            sys.exit("the mod_cf32 graph did not replay the scrambled mapping: " + json.dumps(out))
    for name, t in times.items():
        t_sorted = sorted(t)
        rec = {"us": t, "median": t_sorted[len(t) // 2], "spread": round(max(t) - min(t), 2)}
        if name.startswith("mod_"):
            nbytes = nbits / 8 + out["symbols"] * (8 if name.endswith("cf32") else 2)
            rec["bytes_read_plus_written"] = int(nbytes)
            rec["gb_per_s"] = round(nbytes / rec["median"] / 1e3, 1)
            rec["hbm_peak_gb_per_s"] = 8000
        out[name] = rec
        ctxs[name].lib.ldpc_hip_graph_destroy(graphs[name])
    out["largest_spread_us"] = max(out[n]["spread"] for n in times)
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
