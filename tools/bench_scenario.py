#!/usr/bin/env python3
"""Time of one ace_synth_scenario call at (count 4096, m 256, 32 x 32), shared codebook:

  * at the default cfg, beside ace_synth_channels (the per-realisation product, one work-group per realisation) at the
    same shape in the same process, the two alternating after a warm-up call each;
  * at the Vs_SNR.m cfg (L = 1, rician_k = 5, 40 degrees, combiner noise on the 16 x 16 directional Kronecker codebook).

Device events around each call, `reps` times; the median and the spread (min, max) are reported.  Also the generator's
share of one ``montecarlo.vs_snr`` point (8 x 8, M = 6, one chunk of 64, the given PhaseLift iteration cap): the two
scenario calls of the point timed by events against the point's wall time.

    python tools/bench_scenario.py [--count 4096] [--m 256] [--ant 32] [--reps 9] [--pl-maxits 200]

Prints one JSON line and writes it to --out (default profiles/scenario_bench.json).
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))


def main():
    import numpy as np
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--ant", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pl-maxits", type=int, default=200)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scenario_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scenario needs a GPU")
    from ace_amd import angular, montecarlo, scenario_batch, scenario_cfg, synth_problem
    dev = torch.device("cuda:0")
    count, m, tx = a.count, a.m, a.ant
    n = tx * tx

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(ts):
        ts = sorted(ts)
        return {"ms": round(ts[len(ts) // 2], 4), "ms_min_max": [round(ts[0], 4), round(ts[-1], 4)]}

    A = synth_problem(1, 0, 1, m, tx, tx)[0]                       # the shared phase-code codebook
    synth_old = lambda: synth_problem(1, 0, count, m, tx, tx, A=A)   # noqa: E731  (B, X0, vecH / ||B||)
    want3 = ("B", "X0", "Hn")
    scen_def = lambda: scenario_batch(1, 0, count, tx, tx, A, want=want3)   # noqa: E731  (the same three outputs)
    scen_all = lambda: scenario_batch(1, 0, count, tx, tx, A)   # noqa: E731
    Mb = int(round(np.sqrt(m)))
    beams = angular.sweep_beams(tx, Mb, 40.0)[0] / np.sqrt(tx)
    Ak = torch.from_numpy(angular.kron_codebook(beams, beams)).to(dev)
    Wk = torch.from_numpy(beams).to(dev)
    cfg = scenario_cfg(L=1, rician_k=5, search_deg=40.0, noise_model=1, snr_db=10.0)
    scen_snr = lambda: scenario_batch(1, 0, count, tx, tx, Ak, cfg, Wk)   # noqa: E731
    calls = {"synth_channels": synth_old, "scenario_default_3out": scen_def, "scenario_default_all": scen_all,
             "scenario_vs_snr_cfg_all": scen_snr}
    for c in calls.values():   # warm-up
        c()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(a.reps):    # alternating
        for k, c in calls.items():
            ts[k].append(timed(c))
    res = {"count": count, "m": m, "tx": tx, "rx": tx, "n": n, "reps": a.reps, **{k: stats(v) for k, v in ts.items()}}
    res["synth_channels_over_scenario_default"] = round(res["synth_channels"]["ms"] / res["scenario_default_3out"]["ms"], 3)
    res["product_gflops_default_3out"] = round(8.0 * count * m * n / (res["scenario_default_3out"]["ms"] * 1e-3) * 1e-9, 1)

    # the generator's share of one vs_snr point
    kw = dict(seed=1, chunk=64, pl_maxits=a.pl_maxits)
    montecarlo.vs_snr(8, 8, 6, [10.0], 64, **kw)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    montecarlo.vs_snr(8, 8, 6, [10.0], 64, **kw)
    torch.cuda.synchronize()
    point = (time.perf_counter() - t0) * 1e3
    b8 = angular.sweep_beams(8, 6, 40.0)[0] / np.sqrt(8)
    A8, W8 = torch.from_numpy(angular.kron_codebook(b8, b8)).to(dev), torch.from_numpy(b8).to(dev)
    R8 = synth_problem(1, 0, 1, 36, 8, 8)[0]
    c8 = scenario_cfg(L=1, rician_k=5, search_deg=40.0, noise_model=1, snr_db=10.0)
    c8r = scenario_cfg(L=1, rician_k=5, search_deg=40.0, snr_db=10.0)

    def two():
        scenario_batch(1, 0, 64, 8, 8, A8, c8, W8, want=("vecH", "y", "y_noisy", "B_raw"))
        scenario_batch(1, 0, 64, 8, 8, R8, c8r, want=("vecH", "B", "Hn"))

    two()
    torch.cuda.synchronize()
    gen = stats([timed(two) for _ in range(a.reps)])
    res["vs_snr_point"] = {"shape": "8x8, M 6, count 64, 5 methods", "pl_maxits": a.pl_maxits, "wall_ms": round(point, 1),
                           "scenario_calls_ms": gen["ms"], "scenario_share": round(gen["ms"] / point, 5)}
    print(json.dumps(res), flush=True)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
