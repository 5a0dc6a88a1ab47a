#!/usr/bin/env python3
"""Time of one batched A-optimal selection call (ace_aopt_select_batch) at the shapes a 32 x 32 array would run:
n = 1024, P = 3968 candidates, M = 256 rows, 8 designs and 1 design, beside the numpy restatement
tests/aopt_ref.py (BLAS products) on the same shape on the same host.

Device events around one call each, after a warm-up call, `reps` times; the median and the spread (min, max) are
reported.  A call synchronises its stream once per pass, so the events cover the whole call.  The restatement is
timed once, at --cpu-maxiter passes (default 1: a pass is 256 steps of the same work), and both are also given per
step (a step is one row of one pass of one design).

Algorithmic bytes: a step's first sweep reads F once (16 P n bytes, shared by the up to 8 designs of a tile group)
and a switch's second sweep once more; per design a step reads Minv twice (u, v) and a switch reads it twice more
(u+, v+) and rewrites it (read + write), 16 n^2 bytes each time.  The F reads are counted for max(iters) M first
sweeps and max(switches) second sweeps per group, a lower bound (designs of a group need not switch in the same
steps), so the share of HBM bandwidth (of the measured 6.29 TB/s copy rate) is a lower bound too; F (65 MB here)
fits the Infinity Cache, the inverses of 8 designs (134 MB) fit it as well.

    python tools/bench_aopt.py [--n 1024] [--P 3968] [--M 256] [--designs 8,1] [--reps 5] [--cpu-maxiter 1]

Prints one JSON line per design count and writes them to --out (default profiles/aopt_bench.json).
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))
sys.path.insert(0, str(ROOT / "tests"))

HBM_TBS = 6.29   # measured copy rate of the MI355X's HBM3E (8.0 TB/s nominal)


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--P", type=int, default=3968)
    ap.add_argument("--M", type=int, default=256)
    ap.add_argument("--designs", default="8,1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-maxiter", type=int, default=1, help="passes of the restatement's timed run (0: skip it)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "aopt_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_aopt needs a GPU")
    from ace_amd import design
    import aopt_ref
    dev = torch.device("cuda:0")
    n, P, M = a.n, a.P, a.M
    rng = np.random.default_rng(1)
    F = np.exp(1j * np.pi / 2 * rng.integers(0, 4, (P, n))) / np.sqrt(n)
    counts = [int(v) for v in a.designs.split(",")]
    inits = rng.integers(0, P, (max(counts), M)).astype(np.int32)
    Fd = torch.as_tensor(F, device=dev)
    note = lambda msg: print(f"[bench_aopt] {msg}", file=sys.stderr, flush=True)   # noqa: E731

    cpu = None
    if a.cpu_maxiter > 0:
        t0 = time.perf_counter()
        ref = aopt_ref.aopt_select(F, M, inits[0], maxiter=a.cpu_maxiter, blas=True)
        cpu = time.perf_counter() - t0
        note(f"restatement: {cpu:.1f} s for {ref.iters} pass(es)")
        one = design.aopt_select_batch(Fd, torch.full((1,), M, dtype=torch.int32, device=dev),
                                       torch.as_tensor(inits[:1], device=dev), maxiter=a.cpu_maxiter)
        same_rows = bool(np.array_equal(one.rowlist[0].cpu().numpy(), ref.rowlist))

    results = []
    for D in counts:
        nrows = torch.full((D,), M, dtype=torch.int32, device=dev)
        init = torch.as_tensor(inits[:D], device=dev)
        call = lambda: design.aopt_select_batch(Fd, nrows, init)   # noqa: E731
        out = call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        ts.sort()
        med = ts[len(ts) // 2]
        iters = out.iters.cpu().numpy().astype(np.int64)
        sw = out.switches.cpu().numpy().astype(np.int64)
        steps = int((iters * M).sum())
        f_bytes = 0.0
        for g0 in range(0, D, 8):
            f_bytes += 16.0 * P * n * (int(iters[g0:g0 + 8].max()) * M + int(sw[g0:g0 + 8].max()))
        m_bytes = 16.0 * n * n * float(2 * steps + 4 * sw.sum())
        res = {"n": n, "P": P, "M": M, "designs": D, "reps": a.reps, "call_s": round(med, 4),
               "call_s_min_max": [round(ts[0], 4), round(ts[-1], 4)], "iters": iters.tolist(), "switches": sw.tolist(),
               "status": out.status.cpu().numpy().tolist(), "steps": steps, "us_per_step": round(med * 1e6 / steps, 2),
               "acrit_start_end": out.acrit.cpu().numpy().round(4).tolist(),
               "F_bytes": f_bytes, "Minv_bytes": m_bytes,
               "bytes_per_s_TB": round((f_bytes + m_bytes) / med * 1e-12, 3),
               "share_of_hbm_copy_rate": round((f_bytes + m_bytes) / med * 1e-12 / HBM_TBS, 3)}
        if cpu is not None:
            res.update({"restatement_s": round(cpu, 2), "restatement_passes": int(ref.iters),
                        "restatement_us_per_step": round(cpu * 1e6 / (ref.iters * M), 1),
                        "restatement_rows_equal_gpu_same_passes": same_rows})
        print(json.dumps(res), flush=True)
        results.append(res)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
