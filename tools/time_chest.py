"""GPU box: what the PUSCH DM-RS channel estimation costs, with the equalizer launch of the
same allocation beside it for scale. Device events over graph replays after warm-up, the variants alternating in one
process, several rounds per variant, so the spread of repeated identical measurements stands beside the differences.

Shapes, each on a received grid of 273 PRB x 14 symbols x 4 ports, DM-RS on symbols 2 and 11, estimates for all 14
symbols, both smoothing strategies:

  one273_1x1    one transmission on PRB 0-272, 1 layer on 1 port (1 plane)
  one273_2x4    the same at 2 layers on 4 ports (8 planes)
  sixteen_1x4   16 transmissions of 17 PRB each, 1 layer on 4 ports (64 planes)

  chest_<strategy>_*  ldpc_hip_dmrs_pusch_estimate_launch
  equalize_*          ldpc_hip_equalize_launch on the 12 data symbols of the same allocation, reading the estimates

Each graph holds CHAIN repetitions of its variant; times are per repetition. Every variant has a context of its own: a
launch's table lives in a per-context device buffer that a captured kernel node only points to. After the rounds each
estimator graph's output is compared with an eager launch of the same rows (equal).

--lib NAME times another build of the library (lib/libsrsran_ldpc_hip_NAME.so, `make exp NAME=...`): the variant with the
interpolation recurrence skipped (FLAGS=-DLDPC_HIP_EXP_CHEST_NO_RECURRENCE) shows what the serial chain costs; its
estimates are wrong and it is never shipped.

usage: python tools/time_chest.py [reps] [rounds] [--lib NAME]"""
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from srsran_projectvtlmo_amd import _lib  # noqa: E402

argv = list(sys.argv[1:])
other_lib = "--lib" in argv
if other_lib:
    at = argv.index("--lib")
    _lib.LIB_PATH = _lib.LIB_PATH.with_name(f"libsrsran_ldpc_hip_{argv[at + 1]}.so")
    del argv[at:at + 2]
reps = int(argv[0]) if len(argv) > 0 else 50
rounds = int(argv[1]) if len(argv) > 1 else 5
CHAIN = 10
NRB, NSYM, GRID_PORTS = 273, 14, 4
DMRS_SYMBOLS = (2, 11)


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


def _ok(ctx, rc, what):
    if rc < 0:
        raise RuntimeError(f"{what} failed ({rc}): {ctx.lib.ldpc_hip_last_error(ctx.handle)}")


def main():
    import numpy as np
    import torch

    from srsran_projectvtlmo_amd import equalization as eq
    from srsran_projectvtlmo_amd import signal_processors as sp
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(6)
    nsubc = NRB * 12
    gshape = (GRID_PORTS, NSYM, nsubc)
    # bf16 patterns of moderate size everywhere: exponent 120 .. 129, any sign and mantissa
    h = rng.integers(0, 1 << 16, gshape + (2,)).astype(np.uint32)
    h = (h & 0x807F) | (rng.integers(120, 130, gshape + (2,)).astype(np.uint32) << 7)
    d_grid = torch.from_numpy((h[..., 0] | (h[..., 1] << 16)).astype(np.uint32).view(np.int32)).cuda()
    shapes = {"one273_1x1": ([(0, 273)], 1, 1), "one273_2x4": ([(0, 273)], 2, 4),
              "sixteen_1x4": ([(17 * i, 17 * i + 17) for i in range(16)], 1, 4)}
    sym = np.zeros(NSYM, bool)
    sym[list(DMRS_SYMBOLS)] = True
    data_symbols = [l for l in range(NSYM) if l not in DMRS_SYMBOLS]
    ctxs, variants, graphs, info, outputs = {}, {}, {}, {}, {}
    for shape_name, (allocs, L, P) in shapes.items():
        eshape = (L, P, NSYM, nsubc)
        planes = L * P * len(allocs)
        nrb = sum(e - b for b, e in allocs)
        d_est = torch.zeros(eshape, dtype=torch.int32, device="cuda")
        d_rec = torch.zeros((planes, 8), dtype=torch.int32, device="cuda")
        d_pil = torch.zeros((planes * 6 * 273, 2), dtype=torch.float32, device="cuda")
        for strategy in ("none", "filter"):
            rows = sp.chest_rows()
            for i, (b, e) in enumerate(allocs):
                rb = np.zeros(NRB, bool)
                rb[b:e] = True
                cfg = sp.pusch_config_t(7, 1, sp.TYPE1, 100 + i, False, 1.0, sym, rb, 0, NSYM, L, list(range(P)))
                rows.add(gshape, eshape, cfg, strategy, result_offset=i * L * P, pilots_offset=i * L * P * 6 * 273)
            name = f"chest_{strategy}_{shape_name}"
            ctxs[name] = _lib.Context(0)
            variants[name] = lambda c=ctxs[name], r=rows, e=d_est, q=d_rec, f=d_pil: sp.dmrs_pusch_estimate_launch(
                c, r, d_grid.data_ptr(), e.data_ptr(), q.data_ptr(), s, False, f.data_ptr())
            outputs[name] = (d_est, d_rec, d_pil)
            info[name] = {"planes": planes, "pilots_per_plane_and_symbol": 6 * nrb // len(allocs),
                          "bytes_written": L * P * nrb * 12 * NSYM * 4}
        # the equalizer on the same allocation's data symbols: one segment per transmission and data symbol
        alg = eq.channel_equalizer_algorithm_type.zf
        segs, oo = [], 0
        for b, e in allocs:
            for l in data_symbols:
                segs.append(eq.eq_segment(12 * (e - b), P, L, [0.01] * P, alg, 1.0, sym_offset=l * nsubc + 12 * b,
                                          est_offset=l * nsubc + 12 * b, out_offset=oo, sym_stride=NSYM * nsubc,
                                          est_stride=NSYM * nsubc))
                oo += 12 * (e - b) * L
        arr = eq.eq_descriptors(segs)
        d_out = torch.zeros((oo, 2), dtype=torch.float32, device="cuda")
        d_var = torch.zeros(oo, dtype=torch.float32, device="cuda")
        name = f"equalize_{shape_name}"
        ctxs[name] = _lib.Context(0)
        variants[name] = lambda c=ctxs[name], a=arr, n=len(segs), e=d_est, o=d_out, v=d_var: eq.equalize_launch(
            c, a, d_grid.data_ptr(), e.data_ptr(), o.data_ptr(), v.data_ptr(), s, n)
        outputs[name] = (d_out, d_var)
        info[name] = {"segments": len(segs), "nof_re": oo // L}
    for name, fn in variants.items():
        c = ctxs[name]
        fn()                      # the table uploaded before the capture
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
    out = {"lib": _lib.LIB_PATH.name, "reps": reps, "rounds": rounds, "chain": CHAIN}
    for name, t in times.items():
        # what the timed graph computes: the eager launch's output
        for o in outputs[name]:
            o.zero_()
        ctxs[name].lib.ldpc_hip_graph_launch(graphs[name], s)
        stream.synchronize()
        replay = [o.clone() for o in outputs[name]]
        for o in outputs[name]:
            o.zero_()
        variants[name]()
        stream.synchronize()
        equal = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(replay, outputs[name]))
        equal = equal and int((outputs[name][0].view(torch.int32) != 0).sum()) > 0
        if not equal and not (other_lib and name.startswith("chest_")):
            sys.exit(f"the {name} graph did not replay the eager launch: " + json.dumps(out))
        t_sorted = sorted(t)
        out[name] = dict(info[name], us=t, median=t_sorted[len(t) // 2], spread=round(max(t) - min(t), 2),
                         replay_equals_eager=equal)
        ctxs[name].lib.ldpc_hip_graph_destroy(graphs[name])
    out["largest_spread_us"] = max(out[n]["spread"] for n in times)
    for c in ctxs.values():
        c.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
