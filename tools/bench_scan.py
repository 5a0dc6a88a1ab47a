#!/usr/bin/env python3
"""Rate of the beam scan (ace_beam_scan_batch, one fused kernel) beside the plain torch composition
``y = einsum(conj(W0), X.view, F1)`` -> ``(y.abs() ** 2).flatten(1).topk(K)`` on the same tensors: device events
around `reps` back-to-back calls, after a warm-up of both, the two alternating over `rounds` rounds (the median
round is reported).  Prints one JSON line per shape and writes them to profiles/scan_bench.json.

    python tools/bench_scan.py [--shapes 4096x16x16x49x49x1,...] [--reps 10] [--rounds 5]
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))

PEAK_F64_TF = 78.6   # MI355X f64 matrix peak
SHAPES = "4096x16x16x49x49x1,4096x32x32x95x95x1,4096x32x32x128x128x16"


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
    from ace_amd import beam_scan_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch x d0 x d1 x Q0 x Q1 x K, comma separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "scan_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scan needs a GPU")
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    results = []
    for shape in a.shapes.split(","):
        batch, d0, d1, Q0, Q1, K = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(batch + 7 * d0 + 13 * Q0 + K)
        rnd = lambda *s: torch.randn(s, dtype=torch.complex128, device=dev, generator=gen)   # noqa: E731
        X, W0, F1 = rnd(batch, d0 * d1), rnd(Q0, d0), rnd(Q1, d1)
        Xm = X.view(batch, d1, d0)                    # [b][j][i] = x[i + d0 j]
        W0c = W0.conj().resolve_conj()                # (conjugated once, outside the timed region)
        fused = lambda: beam_scan_batch(X, W0, F1, K)                                                # noqa: E731
        plain = lambda: (torch.einsum("qi,bji,pj->bpq", W0c, Xm, F1).abs() ** 2).flatten(1).topk(K)   # noqa: E731
        out, ref = fused(), plain()
        same_idx = bool((out.top_idx.long() == ref.indices).all().item())
        rel = float(((out.top_pow - ref.values).abs() / ref.values).max().item())
        for fn in (fused, plain):   # warm-up
            _time(fn, 2)
        t_f, t_p = [], []
        for _ in range(a.rounds):
            t_f.append(_time(fused, a.reps))
            t_p.append(_time(plain, a.reps))
        torch.cuda.synchronize()
        flops = 8.0 * batch * (Q1 * d0 * d1 + Q1 * Q0 * d0)
        fused_bytes = 16.0 * (batch * d0 * d1 + Q0 * d0 + Q1 * d1) + 12.0 * batch * K + 4.0 * batch
        # the composition on top of the inputs: T written and read (c128), the map written (c128), read for abs,
        # |y| written and read for the square, the square written and read by topk (f64)
        torch_bytes = fused_bytes + 2 * 16.0 * batch * Q1 * d0 + (16.0 + 16.0 + 4 * 8.0) * batch * Q1 * Q0
        res = {
            "shape": shape, "batch": batch, "d0": d0, "d1": d1, "Q0": Q0, "Q1": Q1, "K": K, "reps": a.reps,
            "rounds": a.rounds,
            "fused_ms": round(med(t_f) * 1e3, 4), "fused_rounds_ms": [round(t * 1e3, 4) for t in t_f],
            "torch_ms": round(med(t_p) * 1e3, 4), "torch_rounds_ms": [round(t * 1e3, 4) for t in t_p],
            "torch_over_fused": round(med(t_p) / med(t_f), 3),
            "algorithmic_flops": flops, "fused_fraction_of_f64_peak": round(flops / med(t_f) / (PEAK_F64_TF * 1e12), 4),
            "fused_bytes_moved": fused_bytes, "torch_bytes_moved": torch_bytes,
            "map_bytes_c128": 16.0 * batch * Q1 * Q0,
            "indices_equal": same_idx, "max_rel_top_pow_difference": rel, "flagged": int((out.status != 0).sum().item())}
        print(json.dumps(res), flush=True)
        results.append(res)
    pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
