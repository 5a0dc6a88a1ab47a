#!/usr/bin/env python3
"""Time of the batched min-L2 ADMM stage (ace_minl2_admm_batch: pinv's setup, then one kernel for the initialisation
and every iteration) beside the plain torch composition of the same work on the same tensors in the same run:
``torch.linalg.pinv(A)``, then per iteration ``U @ S``, ``A @ X``, ``A^H @ Y`` as batched matmuls and elementwise tensor
code for the rest.  The composition advances the batch in lock step, a stopped realisation's state frozen by
``torch.where``, and reads its stop flags back once per iteration (``.all()``), as a host loop has to.  Device events
around ``reps`` back-to-back calls after a warm-up of both, alternating over ``rounds`` rounds (the median round is
reported).  Prints one JSON line per shape and writes them to profiles/minl2_bench.json.

    python tools/bench_minl2.py [--shapes 64x256x1024x20,64x64x256x20,256x256x1024x20] [--reps 2] [--rounds 3]

Shapes are batch x n x m x r, the row form (scale_by_row) at full length (maxiter 500).  Inputs: a phase-code A /
sqrt(n), Gaussian channels at 30 dB, a Gaussian X0.  The third shape is the first at a batch that gives every compute
unit a work-group (one per realisation).  The ratio is recorded, not gated.
"""
import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "2ace-mmwave-channel-estimation_amd"))

SHAPES = "64x256x1024x20,64x64x256x20,256x256x1024x20"


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def torch_stage(A, B, X0, maxiter=500, mu0=1e-3, rho=1.03, tol_rel=1e-4, tol_abs=1e-8):
    """InferADMM, row form, for the batch: A [m][n], B [batch][m], X0 [batch][r][n].  Returns (X [batch][n][r], iters)."""
    import torch
    m, n = A.shape
    nb, r = X0.shape[0], X0.shape[1]
    U = torch.linalg.pinv(A)
    AH = A.conj().t().resolve_conj().contiguous()
    fro = lambda T: T.abs().pow(2).sum(dim=(1, 2)).sqrt()   # noqa: E731

    def rows(Yc, scale):   # normalize_rows / ArgMinY's tail: rows of norm 0 become 1 / sqrt(r)
        D = Yc.abs().pow(2).sum(dim=2).sqrt()
        z = D == 0
        Yc = torch.where(z[:, :, None], torch.full_like(Yc, r ** -0.5), Yc)
        D = torch.where(z, torch.ones_like(D), D)
        return Yc * scale(D)[:, :, None]

    X = X0.transpose(1, 2)                                  # [batch][n][r]
    X = X * (B.norm(dim=1) / fro(A @ X))[:, None, None]
    Y = rows(A @ X, lambda D: B / D)
    AtY = AH @ Y
    M = torch.zeros_like(Y)
    mu = torch.full((nb,), mu0, dtype=torch.float64, device=A.device)
    last = torch.full_like(mu, float("inf"))
    opt = torch.full_like(mu, float("inf"))
    optX = X.clone()
    done = torch.zeros(nb, dtype=torch.bool, device=A.device)
    iters = torch.zeros(nb, dtype=torch.int64, device=A.device)
    for _ in range(maxiter):
        act = ~done
        iters = iters + act
        mu3 = mu[:, None, None]
        Xn = U @ (Y - M / mu3)
        AX = A @ Xn
        Yn = rows(AX + M / mu3, lambda D: (B / D + mu[:, None]) / (1 + mu[:, None]))
        AtYn = AH @ Yn
        J = AX - Yn
        obj = (AX.abs().pow(2).sum(dim=2).sqrt() - B).norm(dim=1)
        better = act & (obj < opt)
        opt = torch.where(better, obj, opt)
        optX = torch.where(better[:, None, None], Xn, optX)
        res_prim, res_dual = fro(J), mu * fro(AtYn - AtY)
        res_comb = (res_prim ** 2 + fro(Yn - Y) ** 2).sqrt()
        nax, ny = fro(AX), fro(Yn)
        mx = torch.maximum(nax, ny)
        stop = ((res_prim < tol_abs * (m * r) ** 0.5 + tol_rel * mx)
                & (res_dual < tol_abs * (n * r) ** 0.5 + tol_rel * fro(AtYn))) \
            | (res_comb < tol_abs * (2 * m * r) ** 0.5 + tol_rel * (mx ** 2 + ny ** 2).sqrt())
        a3 = act[:, None, None]
        Y, AtY, M = torch.where(a3, Yn, Y), torch.where(a3, AtYn, AtY), torch.where(a3, M + mu3 * J, M)
        go = act & ~stop
        mu = torch.where(go & (res_comb > 0.9 * last), mu * rho, mu)
        last = torch.where(go, res_comb, last)
        done = done | stop
        if bool(done.all()):
            break
    return optX, iters


def main():
    import torch
    from ace_amd import minl2_admm_batch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="batch x n x m x r, comma separated")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "minl2_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_minl2 needs a GPU")
    dev = torch.device("cuda:0")
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    results = []
    for shape in a.shapes.split(","):
        batch, n, m, r = (int(v) for v in shape.split("x"))
        gen = torch.Generator(device=dev).manual_seed(batch + 7 * n + 13 * m)
        rnd = lambda *s: torch.randn(s, dtype=torch.complex128, device=dev, generator=gen)   # noqa: E731
        A = (torch.exp(0.5j * torch.pi * torch.randint(0, 4, (m, n), device=dev, generator=gen).double()) / n ** 0.5).contiguous()
        y = rnd(batch, n) @ A.t()
        B = (y + y.abs().pow(2).mean().sqrt() * 10 ** -1.5 * rnd(batch, m)).abs().contiguous()
        X0 = rnd(batch, r, n).contiguous()
        fused = lambda: minl2_admm_batch(A, B, X0, scale_by_row=True)   # noqa: E731
        plain = lambda: torch_stage(A, B, X0)   # noqa: E731
        out = fused()
        Xt, itt = plain()
        torch.cuda.synchronize()
        same = out.iters.long() == itt
        rel = (out.X.transpose(1, 2) - Xt).abs().pow(2).sum(dim=(1, 2)).sqrt() / Xt.abs().pow(2).sum(dim=(1, 2)).sqrt()
        t_f, t_p = [], []
        for _ in range(a.rounds):
            t_f.append(_time(fused, a.reps))
            t_p.append(_time(plain, a.reps))
        its = float(out.iters.double().mean().item())
        res = {"shape": shape, "batch": batch, "n": n, "m": m, "r": r, "form": "row", "maxiter": 500, "reps": a.reps,
               "rounds": a.rounds, "mean_iters": its, "max_iters": int(out.iters.max().item()),
               "iters_equal_fraction": float(same.double().mean().item()),
               "median_rel_X_difference_where_equal": float(rel[same].median().item()) if bool(same.any()) else None,
               "algorithmic_flops": 3 * 8.0 * m * n * r * its * batch,
               "fused_ms": round(med(t_f) * 1e3, 3), "fused_rounds_ms": [round(t * 1e3, 3) for t in t_f],
               "torch_ms": round(med(t_p) * 1e3, 3), "torch_rounds_ms": [round(t * 1e3, 3) for t in t_p],
               "torch_over_fused": round(med(t_p) / med(t_f), 3)}
        print(json.dumps(res), flush=True)
        results.append(res)
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
