"""CPU model of the m-space entry of the unit solve, with and without the fresh-reference rule.

The iterates come from the oracle's own steps (oracle/ace_oracle.py: argmin_y, argmin_z_lowrank, rank_profile); the
model adds the certificate state machine of the GPU path on top of them, per realisation:

  exact certificate (ace_zprox1w.hip, one-wave Z-step): F = Qprev[:, :16]^H E, the r_p largest squared row norms
      summed (vr_p); it passes when vr_p > f_p ||E||^2 (1 + 1e-9) for every profile entry.  Then Z = E, kf_p =
      sqrt(vr_p), kfcum = 0, kfok = 1.  If it fails the eigensolver runs (Qprev <- the eigenvectors of E E^H) and
      kfok = 0.
  perturbation bound (ace_zcommon.hpp::fused_control): cum = kfcum + ||E_i - E_{i-1}||; it passes when
      (kf_p (1 - 1e-12) - cum)^2 > f_p ||E||^2 (1 + 1e-9) for every p.  Then Z = E and kfcum = cum; else the exact
      certificate above runs.
  entry test (ace_i8gemm.hip::gyk_body): the bound with cum = kfcum + room ||E_i - E_{i-1}|| (room = 32); a
      realisation that passes is in m-space form from that iteration on.
  fresh-reference rule: a candidate the entry test refuses, whose test would pass with kfcum = 0, asks for the exact
      certificate at that iteration (at most once in 5 iterations).

Prints, for both policies, the entry iteration (min .. max, mean) and the exact certificates per realisation.

    python tools/recert_model.py [--count 80] [--seed 58659179] [--iters 90]
"""
import argparse
import math
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "oracle"), str(ROOT / "2ace-mmwave-channel-estimation_amd")]

import ace_oracle as O   # noqa: E402

ROOM, GAP = 32.0, 4


def top_q(E):
    """Eigenvectors of E E^H, eigenvalues descending (the Z-step's warm start Q)."""
    H = E @ E.conj().T
    w, U = np.linalg.eigh(0.5 * (H + H.conj().T))
    return U[:, np.argsort(-w, kind="stable")]


def exact_cert(Q, E, rl, fl):
    """(passes, kf) of the Ky Fan certificate of E against the warm-start eigenvectors Q."""
    rn = np.sort(np.sum(np.abs(Q[:, :16].conj().T @ E) ** 2, axis=1))[::-1]
    v = float(np.sum(np.abs(E) ** 2))
    vr = [float(np.sum(rn[:r])) for r in rl]
    return all(a > f * v * (1.0 + 1e-9) for a, f in zip(vr, fl)) and v > 0.0, [math.sqrt(a) for a in vr]


def bound(kf, cum, s0, fl):
    ok = s0 > 0.0
    for k, f in zip(kf, fl):
        lb = k * (1.0 - 1e-12) - cum
        ok = ok and lb > 0.0 and lb * lb > f * s0 * (1.0 + 1e-9)
    return ok


def run(A, U, B, X0, tx, rx, iters, recert, mu0=1e-3, rho=1.03):
    """One realisation, fixed horizon.  Returns (entry iteration or None, exact certificates, requests, failed)."""
    m, n = A.shape
    rl, fl = O.rank_profile(tx, rx, m, n, False)
    X = np.array(X0, np.complex128).reshape(n, 1)
    M, N = np.zeros((m, 1), np.complex128), np.zeros((n, 1), np.complex128)
    nB = float(np.linalg.norm(B))
    X = X * (nB / float(np.linalg.norm(A @ X)))
    Y = O.normalize_rows(A @ X, B, True)
    E = X.reshape((tx, rx), order="F")
    Z = O.argmin_z_lowrank(X, N, 1.0, tx, rx, m, n, False)
    Q = top_q(E)
    mu, last_res = mu0, math.inf
    kf, kfcum, kfok, nzero, avok, opt_obj = [0.0] * len(rl), 0.0, False, True, False, math.inf
    entry, ncert, nreq, nfail, last_req = None, 0, 0, 0, 0
    for it in range(1, iters + 1):
        Y0, Z0 = Y, Z
        X = U @ (A.conj().T @ (Y - M / mu) + (Z - N / mu))
        AX = A @ X
        Y = O.argmin_y(AX, B, M, mu, True)
        Ev = X + N / mu
        E = Ev.reshape((tx, rx), order="F")
        s0, step = float(np.sum(np.abs(Ev) ** 2)), float(np.linalg.norm(X - Z0))
        cand = kfok and avok and opt_obj < math.inf and it >= 2
        want = False
        if entry is None and cand:
            if bound(kf, kfcum + ROOM * step, s0, fl):
                entry = it
            elif recert and bound(kf, ROOM * step, s0, fl) and (last_req == 0 or it - last_req > GAP):
                want, last_req = True, it
                nreq += 1
        if kfok and nzero and not want and bound(kf, kfcum + step, s0, fl):
            same, kfcum = True, kfcum + step
        else:
            same, kfv = exact_cert(Q, E, rl, fl)
            ncert += 1
            nfail += int(want and not same)
            if not same:   # the eigensolver: Q <- the eigenvectors of E E^H; Z = E unless the tail rescaling fires
                Zs = O.argmin_z_lowrank(X, N, mu, tx, rx, m, n, False)
                Q = top_q(E)
                entry = None   # (a realisation that leaves the form enters again later)
            kfok, kf, kfcum = bool(same and nzero), kfv if same else [0.0] * len(rl), 0.0
        # Z = E leaves N' = N + mu (X - E) = 0 (stored as exact zero, RealState::nzero)
        M = M + mu * (AX - Y)
        if same:
            Z, JN, avok = Ev, X - Ev, nzero
            N, nzero = np.zeros_like(N), True
        else:
            Z, JN = Zs, X - Zs
            N, nzero, avok = N + mu * JN, False, False
        obj = float(np.linalg.norm(np.abs(AX[:, 0]) - B))
        opt_obj = min(opt_obj, obj)
        dZ2 = float(np.linalg.norm(Z - Z0)) ** 2
        res_comb = math.sqrt(float(np.linalg.norm(AX - Y)) ** 2 + float(np.linalg.norm(JN)) ** 2
                             + float(np.linalg.norm(Y - Y0)) ** 2 + dZ2)
        if res_comb > last_res * 0.9:   # (fixed horizon: the stop test never exits)
            mu *= rho
        last_res = res_comb
    return entry, ncert, nreq, nfail


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--count", type=int, default=80)
    ap.add_argument("--seed", type=int, default=58659179)
    ap.add_argument("--iters", type=int, default=90)
    ap.add_argument("--tx", type=int, default=32)
    ap.add_argument("--m", type=int, default=256)
    a = ap.parse_args()
    from ace_amd import synth
    A, B, X0, _ = synth.problem(a.seed, 0, a.count, a.m, a.tx, a.tx)
    U = O.make_U(A[0])
    print(f"seed {a.seed}, realisations 0..{a.count - 1}, {a.tx}-ant, m = {a.m}, {a.iters} iterations, room {ROOM:g}")
    print("| policy | entry iteration, min … max (mean) | exact certificates per realisation | requests (failed) |")
    print("|---|---|---|---|")
    for name, rc in (("current rule", False), ("fresh reference on request", True)):
        res = [run(A[0], U, B[b], X0[b], a.tx, a.tx, a.iters, rc) for b in range(a.count)]
        ent = [r[0] for r in res if r[0] is not None]
        miss = a.count - len(ent)
        print(f"| {name} | {min(ent)} … {max(ent)} ({np.mean(ent):.1f})" + (f", {miss} never" if miss else "")
              + f" | {np.mean([r[1] for r in res]):.1f} | {sum(r[2] for r in res)} ({sum(r[3] for r in res)}) |")


if __name__ == "__main__":
    main()
