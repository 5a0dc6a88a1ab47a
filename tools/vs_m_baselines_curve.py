#!/usr/bin/env python3
"""The recovery-quality curve of tools/vs_m_curve.py with its yardsticks: ace_amd.montecarlo.vs_m_baselines over
the reference's M sweep for one method.  Prints one JSON line with the per-M means of Evaluation_H's metrics and
of the baseline columns (perfect-CSI gains, angle errors, the gain at the estimated angles, the beam sweep with
round(sqrt(M))^2 probes) and writes it to profiles/scan_vs_m_baselines_<ant>x<ant>_count<count>.json.

    python tools/vs_m_baselines_curve.py [--ant 16] [--count 256] [--seed 1] [--method A2only]
"""
import argparse
import json
import math
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))


def main():
    import torch
    from ace_amd import engine
    from ace_amd.montecarlo import BASELINES, vs_m_baselines
    ap = argparse.ArgumentParser()
    ap.add_argument("--ant", type=int, default=16)
    ap.add_argument("--count", type=int, default=256)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--maxiter", type=int, default=None)
    ap.add_argument("--method", default="A2only")
    ap.add_argument("--snr", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vs_m_baselines_curve needs a GPU")
    Ms = [int(M) for M in engine.m_sweep(a.ant, a.ant) if math.floor(0.95 * M) >= min(20, M)]
    t0 = time.perf_counter()
    out = vs_m_baselines(a.ant, a.ant, Ms, a.count, method=a.method, seed=a.seed, maxiter=a.maxiter, snr_db=a.snr)
    torch.cuda.synchronize()
    res = {"method": a.method, "ant": a.ant, "count": a.count, "seed": a.seed, "maxiter": a.maxiter or 500,
           "snr_db": a.snr, "M": Ms, "sweep_beams_per_side": [round(math.sqrt(M)) for M in Ms],
           "columns": list(out["columns"]),
           "mean": [[float(f"{v:.6g}") for v in row] for row in out["mean"]],
           "baseline_mean": {k: [float(f"{v:.6g}") for v in out["baseline_mean"][k]] for k in BASELINES},
           "baseline_median": {k: [float(f"{v:.6g}") for v in np.median(out[k], axis=1)] for k in BASELINES},
           "n_degenerate": out["n_degenerate"].tolist(), "seconds": round(time.perf_counter() - t0, 2)}
    print(json.dumps(res), flush=True)
    path = pathlib.Path(a.out or ROOT / "profiles" / f"scan_vs_m_baselines_{a.ant}x{a.ant}_count{a.count}.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
