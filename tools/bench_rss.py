#!/usr/bin/env python3
"""Rate of the held-out RSS evaluator (ace_rss_evaluate_batch, one fused kernel) beside the plain torch
composition ``((X @ CB.T).abs() - rss).abs() / rss`` -> ``mean(1)`` on the same tensors: device events around
`reps` back-to-back calls, after a warm-up of both, the two alternating over `rounds` rounds (the median round
is reported).  Prints one JSON line per shape and writes them to profiles/rss_bench_evaluate.json.

    python tools/bench_rss.py [--shapes 4096x256x3568,4096x1024x3840] [--reps 10] [--rounds 5]
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))

PEAK_F64_TF = 78.6   # MI355X f64 matrix peak


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    import torch
    from ace_amd import evaluate_rss_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x256x3568,4096x1024x3840", help="batch x n x Pt, comma separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rss_bench_evaluate.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rss needs a GPU")
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    results = []
    for shape in a.shapes.split(","):
        batch, n, Pt = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(batch + 7 * n + 13 * Pt)
        X = torch.randn((batch, n), dtype=torch.complex128, device=dev, generator=gen)
        CB = torch.randn((Pt, n), dtype=torch.complex128, device=dev, generator=gen)
        rss = (X @ CB.T).abs() * (1 + 0.1 * torch.rand((batch, Pt), dtype=torch.float64, device=dev, generator=gen))
        out = evaluate_rss_batch(X, CB, rss)
        fused = lambda: evaluate_rss_batch(X, CB, rss, out=out)                         # noqa: E731
        plain = lambda: (((X @ CB.T).abs() - rss).abs() / rss).mean(1)                   # noqa: E731
        agree = float((out.mean_rel - plain()).abs().max().item())
        for fn in (fused, plain):   # warm-up
            _time(fn, 2)
        t_f, t_p = [], []
        for _ in range(a.rounds):
            t_f.append(_time(fused, a.reps))
            t_p.append(_time(plain, a.reps))
        torch.cuda.synchronize()
        flops = 8.0 * Pt * n * batch
        bytes_moved = 16.0 * (batch * n + Pt * n) + 8.0 * batch * Pt + 32.0 * batch   # X, CB, rss read; metrics written
        res = {
            "shape": shape, "batch": batch, "n": n, "Pt": Pt, "reps": a.reps, "rounds": a.rounds,
            "fused_ms": round(med(t_f) * 1e3, 4), "fused_rounds_ms": [round(t * 1e3, 4) for t in t_f],
            "torch_ms": round(med(t_p) * 1e3, 4), "torch_rounds_ms": [round(t * 1e3, 4) for t in t_p],
            "torch_over_fused": round(med(t_p) / med(t_f), 3),
            "algorithmic_flops": flops, "fused_fraction_of_f64_peak": round(flops / med(t_f) / (PEAK_F64_TF * 1e12), 4),
            "fused_bytes_moved": bytes_moved, "fused_GBps": round(bytes_moved / med(t_f) * 1e-9, 1),
            # what the composition writes and re-reads on top: the [batch][Pt] complex product, then f64 temporaries
            "torch_intermediate_bytes": 16.0 * batch * Pt,
            "max_abs_mean_rel_difference": agree, "flagged": int((out.status != 0).sum().item())}
        print(json.dumps(res), flush=True)
        results.append(res)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
