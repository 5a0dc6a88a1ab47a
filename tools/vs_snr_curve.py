#!/usr/bin/env python3
"""The curve over SNR of Numerical_Simulation/main_programs/Vs_SNR.m: ace_amd.montecarlo.vs_snr (one dominant path with
Rician NLOS paths, M x M directional beams over the searching area, the combiner-coloured noise; A2only on a random
phase-code codebook of M^2 rows beside PLOMP, PLGAMP, PerfectPhaseCS and NoisyPhaseCS).  Prints one JSON line with the
per-SNR means of Evaluation_H's metrics and writes it to profiles/vs_snr_<ant>x<ant>_M<M>_count<count>.json.

    python tools/vs_snr_curve.py [--ant 16] [--M 12] [--count 64] [--seed 1] [--snr -10,0,10,20,30] [--search 40]
                                 [--rician 5] [--noise combiner] [--pl-maxits 4000] [--methods A2only,plomp,...]
"""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))


def main():
    import torch
    from ace_amd.montecarlo import VS_SNR_ADMM, VS_SNR_SPARSE, vs_snr
    ap = argparse.ArgumentParser()
    ap.add_argument("--ant", type=int, default=16)
    ap.add_argument("--M", type=int, default=12)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--snr", default="-10,0,10,20,30")
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--rician", type=int, default=5)
    ap.add_argument("--search", type=float, default=40.0)
    ap.add_argument("--on-grid", action="store_true")
    ap.add_argument("--noise", default="combiner", choices=("combiner", "iid"))
    ap.add_argument("--pl-maxits", type=int, default=4000)
    ap.add_argument("--maxiter", type=int, default=None)
    ap.add_argument("--methods", default="A2only,plomp,plgamp,perfect_cs,noisy_cs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vs_snr_curve needs a GPU")
    methods = tuple(a.methods.split(","))
    snrs = [float(v) for v in a.snr.split(",")]
    r6 = lambda v: [[float(f"{x:.6g}") for x in row] for row in v]   # noqa: E731
    t0 = time.perf_counter()
    out = vs_snr(a.ant, a.ant, a.M, snrs, a.count, methods=methods, L=a.L, rician_k=a.rician, search_deg=a.search,
                 on_grid=a.on_grid, noise=a.noise, seed=a.seed, pl_maxits=a.pl_maxits, maxiter=a.maxiter)
    torch.cuda.synchronize()
    res = {"ant": a.ant, "M": a.M, "count": a.count, "seed": a.seed, "L": a.L, "rician_k": a.rician,
           "search_deg": a.search, "on_grid": a.on_grid, "noise": a.noise, "pl_maxits": a.pl_maxits, "snr_db": snrs,
           "mCS": int(out["mCS"]), "columns": list(out["columns"]), "admm": [k for k in methods if k in VS_SNR_ADMM],
           "sparse": [k for k in methods if k in VS_SNR_SPARSE],
           "mean": {k: r6(out["mean"][k]) for k in methods},
           "median_nmse": {k: [float(f"{x:.6g}") for x in np.median(out[k][:, :, 0], axis=1)] for k in methods},
           "n_degenerate": {k: ((out[f"status_{k}"] & 256) != 0).sum(axis=1).tolist() for k in methods},
           "mean_gain_percsi_ana": [float(f"{x:.6g}") for x in out["gain_percsi_ana"].mean(axis=1)],
           "seconds": round(time.perf_counter() - t0, 2)}
    print(json.dumps(res), flush=True)
    path = pathlib.Path(a.out or ROOT / "profiles" / f"vs_snr_{a.ant}x{a.ant}_M{a.M}_count{a.count}.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
