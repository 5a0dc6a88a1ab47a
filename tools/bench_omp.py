#!/usr/bin/env python3
"""Rate of the batched OMP (ace_omp_solve_batch, one kernel for all iterations) beside the plain torch composition
on the same tensors in the same run: per step one ``D.conj().T @ R``, the masked ``argmax``, and
``torch.linalg.lstsq`` on the gathered atoms.  Device events around `reps` back-to-back calls, after a warm-up of
both, the two alternating over `rounds` rounds (the median round is reported).  The composition takes seconds per
realisation where batched complex128 lstsq is slow, so its repetitions can be set apart (--torch-reps /
--torch-rounds) and it can be run on the first --torch-batch realisations only (it treats them independently); the
JSON records what was used and gives both times per realisation.  Progress notes go to stderr.  Prints one JSON line
per shape and writes them to profiles/omp_bench.json.

    python tools/bench_omp.py [--shapes 4096x155x2401x6,...] [--reps 10] [--rounds 5]
                              [--torch-reps 10] [--torch-rounds 5] [--torch-batch N]

Inputs: a complex Gaussian dictionary with unit columns, signals of 6 atoms plus noise at 5 % of the signal, tol = 0.
With kmax beyond the signal's atoms the late picks fit noise (and at kmax = d rounding noise), so the two versions'
indices are compared on the first 6 picks, where the conditions of tests/omp_ref.py hold, and on all of them.
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))

PEAK_F64_TF = 78.6   # MI355X f64 matrix peak
SHAPES = "4096x155x2401x6,4096x155x2401x155,1024x256x9025x64"
NSIG = 6


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def torch_omp(D, DH, Y, kmax):
    """The composition: (idx [batch][kmax], coef [batch][kmax]) at tol = 0."""
    import torch
    batch, d = Y.shape
    R = Y.clone()
    chosen = torch.zeros((batch, D.shape[1]), dtype=torch.bool, device=Y.device)
    idx = torch.empty((batch, kmax), dtype=torch.long, device=Y.device)
    Dt = D.t()                                         # [N][d]: a gathered atom is a row
    c = None
    for k in range(kmax):
        corr = (DH @ R.t()).t()                        # [batch][N]
        p = corr.real ** 2 + corr.imag ** 2
        p[chosen] = -1.0
        j = p.argmax(dim=1)
        idx[:, k] = j
        chosen[torch.arange(batch, device=Y.device), j] = True
        DI = Dt[idx[:, :k + 1]].transpose(1, 2)        # [batch][d][k + 1]
        c = torch.linalg.lstsq(DI, Y.unsqueeze(2)).solution
        R = Y - (DI @ c).squeeze(2)
    return idx, c.squeeze(2)


def main():
    import torch
    from ace_amd import omp_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch x d x N x kmax, comma separated")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=None)
    ap.add_argument("--torch-rounds", type=int, default=None)
    ap.add_argument("--torch-batch", type=int, default=None,
                    help="run the composition on the first TORCH_BATCH realisations only (it treats them independently); "
                         "its time is reported as measured, next to the batch it ran")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "omp_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_omp needs a GPU")
    treps = a.reps if a.torch_reps is None else a.torch_reps
    trounds = a.rounds if a.torch_rounds is None else a.torch_rounds
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    results = []
    for shape in a.shapes.split(","):
        batch, d, N, kmax = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(batch + 7 * d + 13 * N + kmax)
        rnd = lambda *s: torch.randn(s, dtype=torch.complex128, device=dev, generator=gen)   # noqa: E731
        D = rnd(d, N)
        D = (D / D.abs().pow(2).sum(dim=0).sqrt()).contiguous()
        sup = torch.rand((batch, N), device=dev, generator=gen).argsort(dim=1)[:, :NSIG]
        sig = (D.t()[sup] * (1.0 + torch.rand((batch, NSIG, 1), device=dev, generator=gen, dtype=torch.float64))
               * torch.exp(2j * torch.pi * torch.rand((batch, NSIG, 1), device=dev, generator=gen, dtype=torch.float64))).sum(dim=1)
        Y = (sig + 0.05 * sig.abs().pow(2).sum(dim=1, keepdim=True).sqrt() / d ** 0.5 * rnd(batch, d) * 0.5 ** 0.5).contiguous()
        DH = D.conj().t().resolve_conj().contiguous()   # (conjugated once, outside the timed region)
        fused = lambda: omp_batch(D, Y, kmax, 0.0)      # noqa: E731
        tb = batch if a.torch_batch is None else min(batch, a.torch_batch)
        Yt = Y[:tb].contiguous()
        plain = lambda: torch_omp(D, DH, Yt, kmax)      # noqa: E731
        note = lambda msg: print(f"[bench_omp {shape}] {msg}", file=sys.stderr, flush=True)   # noqa: E731
        out = fused()
        torch.cuda.synchronize()
        note("fused ran")
        res = {"shape": shape, "batch": batch, "d": d, "N": N, "kmax": kmax, "reps": a.reps, "rounds": a.rounds,
               "torch_reps": treps, "torch_rounds": trounds, "torch_batch": tb}
        try:
            ridx, rcoef = plain()
            torch.cuda.synchronize()
            note("composition ran")
            kc = min(kmax, NSIG)
            eq_first = (out.idx[:tb, :kc].long() == ridx[:, :kc]).all(dim=1)
            eq_all = (out.idx[:tb].long() == ridx).all(dim=1)
            res.update({"indices_equal_first6_fraction": float(eq_first.double().mean().item()),
                        "indices_equal_all_fraction": float(eq_all.double().mean().item()),
                        "max_rel_coef_difference_where_equal":
                            float(((out.coef[:tb] - rcoef).abs().amax(dim=1) / rcoef.abs().amax(dim=1))[eq_all].max().item())
                            if bool(eq_all.any()) else None})
            torch_ok = True
        except Exception as e:   # the composition is the yardstick, not the product: report, do not hide
            res["torch_error"] = f"{type(e).__name__}: {e}"[:300]
            torch_ok = False
        note(f"fused warm-up {_time(fused, 2) * 1e3:.2f} ms per call")
        if torch_ok:
            note(f"composition warm-up {_time(plain, 1) * 1e3:.1f} ms per call")
        t_f, t_p = [], []
        for r in range(max(a.rounds, trounds if torch_ok else 0)):
            if r < a.rounds:
                t_f.append(_time(fused, a.reps))
            if torch_ok and r < trounds:
                t_p.append(_time(plain, treps))
        torch.cuda.synchronize()
        steps = float(out.count.double().mean().item())
        nblk = (batch + 15) // 16
        # 8 flop per complex multiply-add: the correlations, and per step k the orthogonalisation (k d), the
        # projection of r (d) twice over (dot and update)
        corr_flops = 8.0 * batch * steps * N * d
        ls_flops = 8.0 * batch * 2.0 * d * (steps * (steps - 1) / 2 + steps)
        # bytes: every work-group streams D once per step (from L2 / Infinity Cache; D itself is 16 d N bytes of
        # HBM once); a realisation reads its Q rows once per step and writes one; inputs and outputs once
        fused_bytes = 16.0 * d * N * nblk * steps + 16.0 * d * batch * (steps * (steps - 1) / 2 + steps) \
            + 16.0 * batch * d + (16.0 + 4.0) * batch * kmax
        # the composition per step: D read, R read, the correlations written, read for the squares, the squares
        # written and read (f64), the gathered atoms written and read by lstsq (its own workspace not counted), R written
        # (for the batch the composition ran)
        torch_bytes = steps * (16.0 * d * N + 2 * 16.0 * tb * d + (2 * 16.0 + 2 * 8.0) * tb * N) \
            + 2 * 16.0 * tb * d * (steps * (steps + 1) / 2)
        res.update({
            "fused_ms": round(med(t_f) * 1e3, 4), "fused_rounds_ms": [round(t * 1e3, 4) for t in t_f],
            "mean_steps": steps, "flagged": int((out.status != 0).sum().item()),
            "algorithmic_flops": corr_flops + ls_flops, "correlation_flops": corr_flops,
            "fused_fraction_of_f64_peak": round((corr_flops + ls_flops) / med(t_f) / (PEAK_F64_TF * 1e12), 4),
            "fused_bytes_moved": fused_bytes, "fused_D_stream_bytes": 16.0 * d * N * nblk * steps,
            "torch_bytes_moved": torch_bytes})
        if torch_ok:
            # per realisation, so that a composition run on a part of the batch compares like with like
            res.update({"torch_ms": round(med(t_p) * 1e3, 4), "torch_rounds_ms": [round(t * 1e3, 4) for t in t_p],
                        "torch_us_per_realisation": round(med(t_p) * 1e6 / tb, 3),
                        "fused_us_per_realisation": round(med(t_f) * 1e6 / batch, 3),
                        "torch_over_fused_per_realisation": round((med(t_p) / tb) / (med(t_f) / batch), 3),
                        "torch_fraction_of_f64_peak":
                            round((corr_flops + ls_flops) * tb / batch / med(t_p) / (PEAK_F64_TF * 1e12), 5)})
        print(json.dumps(res), flush=True)
        results.append(res)
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
