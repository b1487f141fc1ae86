"""GPU box: what PUSCH descrambling costs. Device events over graph replays after warm-up,
the variants alternating in one process:

  slot        the C4 slot from symbols (bench.extra_c4's workload), scrambling off / on (every TB scrambled, descrambled
              inside the fused dematcher) / on with the stand-alone kernels (fuse_demod = False: demodulate, descramble
              in place, dematch + decode); end-to-end slot times (demodulate .. TB join), several rounds per variant,
              so the spread of repeated identical measurements stands beside the differences
  descramble  ldpc_hip_descramble_launch over one C4 slot's worth of LLRs (one segment per TB): kernel time and GB/s of
              LLR traffic (read + write)

The library is chosen as tools/batch_time_lib.py does (LIB_SUFFIX, '-' for the product library), so the same script
times the scrambling-off slot on a build of the parent commit (that library has no scrambling entry points: only the
"off" variant runs on it).

usage: python tools/time_scramble.py LIB_SUFFIX|- [reps] [rounds]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from srsran_projectvtlmo_amd import _lib  # noqa: E402

if len(sys.argv) < 2:
    sys.exit(__doc__)
if sys.argv[1] != "-":
    _lib.LIB_PATH = ROOT / "srsran_projectvtlmo_amd" / "lib" / f"libsrsran_ldpc_hip_{sys.argv[1]}.so"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5


def c4_pipeline(ctx, scrambled: bool, seed=3):
    """bench.extra_c4(from_symbols=True)'s slot; scrambled: every TB with its own (rnti, n_id)."""
    import numpy as np

    from srsran_projectvtlmo_amd import pusch
    from srsran_projectvtlmo_amd import segmentation as S
    from srsran_projectvtlmo_amd import synth
    rng = np.random.default_rng(seed)
    ues = [(1078248, 1, 250 * 156 * 4, 8, 4)] + [(256, 2, 156 * 4, 2, 4)] * 23
    specs, syms = [], []
    for k, (tbs, bg, nsym, qm, layers) in enumerate(ues):
        metas = S.segment_rx(tbs, bg, nsym, qm, layers)
        m0 = metas[0]
        msgs = S.segment_tx(rng.integers(0, 2, tbs).astype(np.uint8), metas)
        kw = {"rnti": 0x4601 + k, "n_id": 17 * k} if scrambled else {}
        specs.append(pusch.tb_slot_spec(tbs, bg, m0.lifting_size, m0.nof_filler_bits, [m.rm_length for m in metas],
                                        qm, 0, True, 0, 8, True, **kw))
        skw = {"c_init": ((0x4601 + k) << 15) + 17 * k} if scrambled else {}
        syms.append(synth.rate_matched_symbols(ctx, bg, m0.lifting_size, msgs, [m.rm_length for m in metas], qm, 0,
                                               m0.nof_filler_bits, 0.0015 if qm == 8 else 0.1, seed=seed + k, **skw))
    pipe = pusch.SlotPipeline(ctx, specs)
    pipe.upload_symbols_device([a for a, _ in syms], [b for _, b in syms])
    return pipe


def main():
    import torch

    import bench
    has_scr = hasattr(_lib.ctypes.CDLL(str(_lib.LIB_PATH)), "ldpc_hip_descramble_launch")
    if not has_scr:
        # the parent commit's library: the binding finds every other entry point; the scrambling ones stay unbound
        import ctypes
        import types

        class parent_library(ctypes.CDLL):
            def __getattr__(self, name):
                try:
                    return super().__getattr__(name)
                except AttributeError:
                    if "_prs_" in name or "scr" in name:
                        return types.SimpleNamespace()
                    raise
        ctypes.CDLL = parent_library
    ctx = _lib.Context(0)
    stream = torch.cuda.Stream()
    out = {"lib": _lib.LIB_PATH.name, "reps": reps, "rounds": rounds}
    variants = {"off": c4_pipeline(ctx, False)}
    if has_scr:
        variants["on_fused"] = c4_pipeline(ctx, True)
        variants["on_separate"] = c4_pipeline(ctx, True)
        variants["on_separate"].fuse_demod = False
        variants["off_separate"] = c4_pipeline(ctx, False)
        variants["off_separate"].fuse_demod = False
    for name, p in variants.items():
        p.capture(stream.cuda_stream)
        bench._time(lambda: p.launch_graph(stream.cuda_stream), stream, reps)  # warm-up
    times = {name: [] for name in variants}
    for _ in range(rounds):  # alternate the variants
        for name, p in variants.items():
            times[name].append(round(bench._time(lambda: p.launch_graph(stream.cuda_stream), stream, reps), 2))
    for name, p in variants.items():
        got, cbres = p.results()
        out[f"slot_{name}"] = {"us_per_slot_graph": times[name], "min": min(times[name]), "max": max(times[name]),
                               "tb_crc_ok": int(sum(1 for g in got if g[1])), "tbs": len(got),
                               "mean_iterations": round(float(cbres[:, 1].mean()), 3)}
        p.release_graph()
    if has_scr:
        from srsran_projectvtlmo_amd import sequence_generators as sg
        p = variants["on_fused"]
        n = sum(sum(tb.rm_lengths) for tb in p.tbs)
        # one segment per TB (a codeword is one contiguous run of the sequence); 16-byte aligned starts
        segs, o = [], 0
        for tb in p.tbs:
            e = sum(tb.rm_lengths)
            segs.append(sg.prs_segment(e, sg.pusch_c_init(tb.rnti, tb.n_id), 0, o, o))
            o += (e + 15) // 16 * 16
        d = torch.randint(-127, 128, (o,), dtype=torch.int8, device="cuda")
        arr = sg.prs_descriptors(segs)
        fn = lambda: sg.descramble_launch(ctx, arr, d.data_ptr(), d.data_ptr(), stream.cuda_stream, n=len(segs))  # noqa
        fn()
        stream.synchronize()
        _lib.check(ctx.handle, ctx.lib.ldpc_hip_capture_begin(ctx.handle, stream.cuda_stream), "capture_begin")
        for _ in range(10):
            fn()
        g = _lib.ctypes.c_void_p()
        _lib.check(ctx.handle, ctx.lib.ldpc_hip_capture_end(ctx.handle, stream.cuda_stream, _lib.ctypes.byref(g)),
                   "capture_end")
        us = [round(bench._time(lambda: ctx.lib.ldpc_hip_graph_launch(g, stream.cuda_stream), stream, reps) / 10, 2)
              for _ in range(rounds)]
        ctx.lib.ldpc_hip_graph_destroy(g)
        out["descramble_kernel"] = {"llrs": n, "us": us, "gb_per_s_read_plus_write": round(2 * n / min(us) / 1e3, 1),
                                    "hbm_peak_gb_per_s": 8000}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
