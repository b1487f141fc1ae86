"""GPU box: what layer mapping and precoding into the grid cost. Device events over graph
replays after warm-up, the variants alternating in one process, several rounds per variant, so the spread of repeated
identical measurements stands beside the differences.

Workload: the downlink mirror of C4, a grid of 273 PRB x 14 symbols x 4 ports: one 4-layer transmission on PRB 0-249
and 23 one-PRB 4-layer transmissions on PRB 250-272, each on 13 data symbols (symbol 2 is a DM-RS symbol without
data): 24 x 13 = 312 rows, 42,588 REs, 2 L = 8 bytes of ci8 symbols in and 4 P = 16 bytes of cbf16 out per RE.

  wideband  one PRG per transmission
  prg4      prg_size 4: 69 PRGs per transmission

Each graph holds CHAIN repetitions of its variant; times are per repetition. Every variant has a context of its own: a
launch's table lives in a per-context device buffer that a captured kernel node only points to. After the rounds each
graph's grid is compared with an eager launch of the same rows (equal).

usage: python tools/time_precode.py [reps] [rounds]"""
import ctypes
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from srsran_projectvtlmo_amd import _lib  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
CHAIN = 10
NRB, NSYM, PORTS, LAYERS = 273, 14, 4, 4
DMRS_SYMBOL = 2


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

    from srsran_projectvtlmo_amd import precoding as pc
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(5)
    nsubc = NRB * 12
    shape = (PORTS, NSYM, nsubc)
    allocs = [(0, 250)] + [(b, b + 1) for b in range(250, NRB)]
    nof_re = sum(e - b for b, e in allocs) * 12 * (NSYM - 1)
    d_sym = torch.from_numpy((2 * rng.integers(0, 8, (nof_re * LAYERS, 2)) - 7).astype(np.int8)).cuda()
    d_grid = torch.zeros(shape, dtype=torch.int32, device="cuda")
    ctxs, variants, graphs, nrows = {}, {}, {}, {}
    for name, prg_size in (("wideband", 275), ("prg4", 4)):
        c = ctxs[name] = _lib.Context(0)
        nprg = 1 if prg_size == 275 else -(-NRB // prg_size)
        rows, so = pc.precode_rows(), 0
        for b, e in allocs:
            masks = np.zeros((NSYM, nsubc), bool)
            masks[:, 12 * b:12 * e] = True
            masks[DMRS_SYMBOL] = False
            w = (rng.integers(-64, 65, (nprg, PORTS, LAYERS, 2)) / 37).astype(np.float32).view(np.complex64)[..., 0]
            so += LAYERS * rows.add(shape, masks, prg_size, w, 1 / np.sqrt(42), sym_offset=so)
        assert so == nof_re * LAYERS
        nrows[name] = len(rows.rows)
        variants[name] = lambda c=c, rows=rows: pc.precode_map_launch(c, rows, d_sym.data_ptr(), d_grid.data_ptr(), s)
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
    out = {"lib": _lib.LIB_PATH.name, "reps": reps, "rounds": rounds, "chain": CHAIN, "nof_re": nof_re,
           "rows": nrows}
    nbytes = nof_re * (2 * LAYERS + 4 * PORTS)
    for name, t in times.items():
        # what the timed graph computes: the eager launch's grid
        d_grid.zero_()
        ctxs[name].lib.ldpc_hip_graph_launch(graphs[name], s)
        stream.synchronize()
        replay = d_grid.clone()
        d_grid.zero_()
        variants[name]()
        stream.synchronize()
        equal = bool(torch.equal(replay, d_grid)) and int((d_grid != 0).sum()) > nof_re * PORTS // 2
        if not equal:
            sys.exit(f"the {name} graph did not replay the eager launch: " + json.dumps(out))
        t_sorted = sorted(t)
        rec = {"us": t, "median": t_sorted[len(t) // 2], "spread": round(max(t) - min(t), 2),
               "replay_equals_eager": equal, "bytes_read_plus_written": nbytes}
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
