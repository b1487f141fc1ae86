"""GPU box: what PDSCH DM-RS generation and mapping into the grid cost, with the precoder
launch on the same grid beside it for scale. Device events over graph replays after warm-up, the variants alternating
in one process, several rounds per variant, so the spread of repeated identical measurements stands beside the
differences.

Shapes, each on a grid of 273 PRB x 14 symbols x 4 ports, type 1, 4 layers on 4 ports, DM-RS on symbols 2 and 11:

  one273   one transmission on PRB 0-272
  sixteen  16 transmissions of 17 PRB each (PRB 0-271)

  dmrs_*     ldpc_hip_dmrs_pdsch_map_launch: 2 rows per transmission, 12 cbf16 REs per RB, symbol and port
  precode_*  ldpc_hip_precode_map_launch of the same transmissions' data: the 12 other symbols (with 4 layers both CDM
             groups are taken, so a DM-RS symbol carries no data)

Each graph holds CHAIN repetitions of its variant; times are per repetition. Every variant has a context of its own: a
launch's table lives in a per-context device buffer that a captured kernel node only points to. After the rounds each
graph's grid is compared with an eager launch of the same rows (equal).

usage: python tools/time_dmrs.py [reps] [rounds]"""
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

    from srsran_projectvtlmo_amd import precoding as pc
    from srsran_projectvtlmo_amd import signal_processors as sp
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(6)
    nsubc = NRB * 12
    shape = (PORTS, NSYM, nsubc)
    d_grid = torch.zeros(shape, dtype=torch.int32, device="cuda")
    shapes = {"one273": [(0, 273)], "sixteen": [(17 * i, 17 * i + 17) for i in range(16)]}
    sym = np.zeros(NSYM, bool)
    sym[list(DMRS_SYMBOLS)] = True
    ctxs, variants, graphs, info, keep = {}, {}, {}, {}, []
    for shape_name, allocs in shapes.items():
        nrb = sum(e - b for b, e in allocs)
        data_re = nrb * 12 * (NSYM - len(DMRS_SYMBOLS))
        d_sym = torch.from_numpy((2 * rng.integers(0, 8, (data_re * LAYERS, 2)) - 7).astype(np.int8)).cuda()
        keep.append(d_sym)
        drows, prows, so = sp.dmrs_rows(), pc.precode_rows(), 0
        for i, (b, e) in enumerate(allocs):
            w = (rng.integers(-64, 65, (1, PORTS, LAYERS, 2)) / 37).astype(np.float32).view(np.complex64)[..., 0]
            rb = np.zeros(NRB, bool)
            rb[b:e] = True
            drows.add(shape, sp.config_t(7, 0, sp.TYPE1, 100 + i, False, 1.0, sym, rb, w[0]))
            masks = np.zeros((NSYM, nsubc), bool)
            masks[:, 12 * b:12 * e] = True
            masks[list(DMRS_SYMBOLS)] = False
            so += LAYERS * prows.add(shape, masks, 275, w, 1 / np.sqrt(42), sym_offset=so)
        assert so == data_re * LAYERS
        cd, cp = _lib.Context(0), _lib.Context(0)
        ctxs["dmrs_" + shape_name], ctxs["precode_" + shape_name] = cd, cp
        variants["dmrs_" + shape_name] = lambda c=cd, r=drows: sp.dmrs_pdsch_map_launch(c, r, d_grid.data_ptr(), s)
        variants["precode_" + shape_name] = lambda c=cp, r=prows, x=d_sym: pc.precode_map_launch(
            c, r, x.data_ptr(), d_grid.data_ptr(), s)
        dmrs_re = nrb * 12 * len(DMRS_SYMBOLS)
        info["dmrs_" + shape_name] = {"rows": len(allocs) * len(DMRS_SYMBOLS), "nof_re": dmrs_re,
                                      "bytes_written": dmrs_re * 4 * PORTS}
        info["precode_" + shape_name] = {"rows": len(prows.rows), "nof_re": data_re,
                                         "bytes_read_plus_written": data_re * (2 * LAYERS + 4 * PORTS)}
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
        # what the timed graph computes: the eager launch's grid
        d_grid.zero_()
        ctxs[name].lib.ldpc_hip_graph_launch(graphs[name], s)
        stream.synchronize()
        replay = d_grid.clone()
        d_grid.zero_()
        variants[name]()
        stream.synchronize()
        equal = bool(torch.equal(replay, d_grid)) and int((d_grid != 0).sum()) > info[name]["nof_re"] * PORTS // 2
        if not equal:
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
