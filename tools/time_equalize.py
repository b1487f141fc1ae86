"""GPU box: what the channel equalizer costs. Device events over graph replays after warm-up,
the variants alternating in one process, several rounds per variant, so the spread of repeated identical measurements
stands beside the differences.

Workload: the C4 grid's 42,588 REs (273 PRB x 12 subcarriers x 13 data symbols) as one segment, random finite cbf16
REs and estimates (the kernel's time does not depend on the values, apart from the abnormal REs' early exit, of which
there are none here):

  zf_2x4    ZF, 2 layers on 4 ports   (PUSCH MIMO; 4 P (1 + L) = 48 bytes in and 12 L = 24 bytes out per RE)
  zf_1x4    ZF, 1 layer on 4 ports    (32 in, 12 out)
  mmse_1x4  MMSE, 1 layer on 4 ports  (32 in, 12 out)

Each graph holds CHAIN repetitions of its variant; times are per repetition. Every variant has a context of its own: a
launch's descriptor table lives in a per-context device buffer that a captured kernel node only points to. After the
rounds the zf_2x4 graph's output is compared with an eager launch of the same descriptors (equal).

usage: python tools/time_equalize.py [reps] [rounds]"""
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
NOF_RE = 273 * 12 * 13


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
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    rng = np.random.default_rng(5)

    def planes(k):  # finite bf16 patterns, magnitudes 2^-7 .. 2^3
        d = rng.integers(0, 1 << 16, (k, NOF_RE, 2))
        e = rng.integers(120, 131, (k, NOF_RE, 2))
        return torch.from_numpy((((d & 0x8000) | (e << 7) | (d & 0x7F)).astype(np.uint16)).view(np.int16)).cuda()

    d_sym, d_est = planes(4), planes(8)
    d_out = torch.zeros(2 * 2 * NOF_RE, dtype=torch.float32, device="cuda")
    d_var = torch.zeros(2 * NOF_RE, dtype=torch.float32, device="cuda")
    nv = [0.01, 0.012, 0.009, 0.011]
    shapes = {"zf_2x4": (0, 4, 2), "zf_1x4": (0, 4, 1), "mmse_1x4": (1, 4, 1)}
    ctxs, variants, graphs = {}, {}, {}
    for name, (alg, P, L) in shapes.items():
        c = ctxs[name] = _lib.Context(0)
        arr = eq.eq_descriptors([eq.eq_segment(NOF_RE, P, L, nv[:P], alg, 1.0)])
        variants[name] = lambda c=c, arr=arr: eq.equalize_launch(c, arr, d_sym.data_ptr(), d_est.data_ptr(),
                                                                 d_out.data_ptr(), d_var.data_ptr(), s, n=1)
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
    out = {"lib": _lib.LIB_PATH.name, "reps": reps, "rounds": rounds, "chain": CHAIN, "nof_re": NOF_RE}
    # what the timed zf_2x4 graph computes: the eager launch's output
    ctxs["zf_2x4"].lib.ldpc_hip_graph_launch(graphs["zf_2x4"], s)
    stream.synchronize()
    replay = (d_out.clone(), d_var.clone())
    d_out.zero_()
    d_var.zero_()
    variants["zf_2x4"]()
    stream.synchronize()
    out["zf_2x4_replay_equals_eager"] = bool(torch.equal(replay[0].view(torch.int32), d_out.view(torch.int32)) and
                                             torch.equal(replay[1].view(torch.int32), d_var.view(torch.int32)))
    out["zf_2x4_finite_variances"] = int(torch.isfinite(d_var).sum())
    if not out["zf_2x4_replay_equals_eager"]:
        sys.exit("the zf_2x4 graph did not replay the eager launch: " + json.dumps(out))
    for name, t in times.items():
        alg, P, L = shapes[name]
        t_sorted = sorted(t)
        rec = {"us": t, "median": t_sorted[len(t) // 2], "spread": round(max(t) - min(t), 2)}
        nbytes = NOF_RE * (4 * P * (1 + L) + 12 * L)
        rec["bytes_read_plus_written"] = nbytes
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
