#!/usr/bin/env python3
"""Recovery-quality curve of the build: ace_amd.montecarlo.vs_m over the reference's M sweep
(round(linspace(2, sqrt(4 tx rx), 8))^2, without the points the pipeline refuses) for A2only and
A2nuclear.  Prints one JSON line per method with the per-M means of Evaluation_H's metrics.

    python tools/vs_m_curve.py [--ant 16] [--count 256] [--seed 1] [--maxiter 500]
"""
import argparse
import json
import math
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))


def main():
    import torch
    from ace_amd import engine
    from ace_amd.montecarlo import vs_m
    ap = argparse.ArgumentParser()
    ap.add_argument("--ant", type=int, default=16)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--maxiter", type=int, default=None)
    ap.add_argument("--methods", default="A2only,A2nuclear")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vs_m_curve needs a GPU")
    Ms = [int(M) for M in engine.m_sweep(a.ant, a.ant) if math.floor(0.95 * M) >= min(20, M)]
    for method in a.methods.split(","):
        t0 = time.perf_counter()
        out = vs_m(a.ant, a.ant, Ms, a.count, method=method, seed=a.seed, maxiter=a.maxiter)
        torch.cuda.synchronize()
        print(json.dumps({
            "method": method, "ant": a.ant, "count": a.count, "seed": a.seed, "maxiter": a.maxiter or 500,
            "M": Ms, "columns": list(out["columns"]),
            "mean": [[float(f"{v:.6g}") for v in row] for row in out["mean"]],
            "n_degenerate": out["n_degenerate"].tolist(),
            "seconds": round(time.perf_counter() - t0, 2)}), flush=True)


if __name__ == "__main__":
    main()
