#!/usr/bin/env python3
"""The sparse recoveries' curve next to tools/vs_m_curve.py's: ace_amd.montecarlo.vs_m_sparse (PLOMP with
max_atoms = mCS and = 2 s, PerfectPhaseCS where M <= 256), with --prgamp the direct PR-GAMP baseline (M <= 256) and,
with --admm, vs_m for A2only on the same realisations.
Prints one JSON line with the per-M means of Evaluation_H's metrics and writes it to
profiles/omp_vs_m_sparse_<ant>x<ant>_count<count>.json.

    python tools/vs_m_sparse_curve.py [--ant 16] [--count 64] [--seed 1] [--M 64,121,256] [--pl-maxits 4000] [--admm]
                                     [--prgamp] [--max-try 100]
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
    from ace_amd.montecarlo import SPARSE, vs_m, vs_m_sparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--ant", type=int, default=16)
    ap.add_argument("--count", type=int, default=64)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--M", default="64,121,256,400")
    ap.add_argument("--L", type=int, default=3)
    ap.add_argument("--snr", type=float, default=30.0)
    ap.add_argument("--pl-maxits", type=int, default=4000)
    ap.add_argument("--admm", action="store_true", help="also run vs_m (A2only) on the same realisations")
    ap.add_argument("--prgamp", action="store_true", help="also run the PR-GAMP baseline (Method.PRGAMP)")
    ap.add_argument("--max-try", type=int, default=100, help="PR-GAMP restarts per realisation (the reference's 100)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vs_m_sparse_curve needs a GPU")
    Ms = [int(v) for v in a.M.split(",")]
    r6 = lambda v: [[float(f"{x:.6g}") for x in row] for row in v]   # noqa: E731
    t0 = time.perf_counter()
    out = vs_m_sparse(a.ant, a.ant, Ms, a.count, seed=a.seed, L=a.L, snr_db=a.snr, pl_maxits=a.pl_maxits,
                      prgamp=a.prgamp, max_try=a.max_try)
    torch.cuda.synchronize()
    res = {"ant": a.ant, "count": a.count, "seed": a.seed, "L": a.L, "s": out["s"], "snr_db": a.snr,
           "pl_maxits": a.pl_maxits, "M": Ms, "mCS": out["mCS"].tolist(), "columns": list(out["columns"]),
           "mean": {k: r6(out["mean"][k]) for k in SPARSE},
           "median_nmse": {k: [float(f"{x:.6g}") for x in np.median(out[k][:, :, 0], axis=1)] for k in SPARSE},
           "mean_count": {k: out[f"count_{k}"].mean(axis=1).tolist() for k in SPARSE},
           "n_degenerate": {k: ((out[f"status_{k}"] & 256) != 0).sum(axis=1).tolist() for k in SPARSE},
           "n_dependent": {k: ((out[f"status_{k}"] & 1024) != 0).sum(axis=1).tolist() for k in SPARSE},
           "sparse_seconds": round(time.perf_counter() - t0, 2)}
    if a.prgamp:
        res["max_try"] = a.max_try
        res["mean"]["prgamp"] = r6(out["mean"]["prgamp"])
        res["median_nmse"]["prgamp"] = [float(f"{x:.6g}") for x in np.median(out["prgamp"][:, :, 0], axis=1)]
        res["mean_tries_prgamp"] = out["tries_prgamp"].mean(axis=1).tolist()
        res["n_failed_prgamp"] = ((out["status_prgamp"] & 16384) != 0).sum(axis=1).tolist()
        res["n_maxtry_prgamp"] = ((out["status_prgamp"] & 32768) != 0).sum(axis=1).tolist()
    if a.admm:
        t1 = time.perf_counter()
        adm = vs_m(a.ant, a.ant, Ms, a.count, method="A2only", seed=a.seed, L=a.L, snr_db=a.snr)
        torch.cuda.synchronize()
        res["mean"]["A2only"] = r6(adm["mean"])
        res["median_nmse"]["A2only"] = [float(f"{x:.6g}") for x in np.median(adm["metrics"][:, :, 0], axis=1)]
        res["admm_seconds"] = round(time.perf_counter() - t1, 2)
    print(json.dumps(res), flush=True)
    path = pathlib.Path(a.out or ROOT / "profiles" / f"omp_vs_m_sparse_{a.ant}x{a.ant}_count{a.count}.json")
    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
