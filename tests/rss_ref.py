"""References and derived tolerances for the held-out RSS evaluator (ace_rss_evaluate_batch, csrc/ace_rsseval.hip):
tests/test_gpu_rss.py and tests/test_gpu_realtrace.py compare against them, tests/test_rss_ref.py tests them on
the CPU.  Not collected.

    pred_p = |sum_k CB[p][k] X[b][k]|        rel_p = |pred_p - rss_p| / rss_p
    metrics = {mean, rms, max of rel_p over the usable rows, their number}

``evaluate_rss``  the plain numpy (f64) restatement of Evaluate_rss.m with the library's skip and degenerate rules.
``exact``         the same with the product evaluated without rounding (tests/linop_ref.py: sliced-integer
                  planes, recombined in Python integers, returned as hi + lo), the modulus and the statistics in
                  numpy's longdouble (64-bit mantissa on x86: 2^-11 of the f64 unit roundoff, below every
                  tolerance here by that factor).

Tolerance of pred (u = 2^-53, S_p = sum_k |CB[p][k]| |X[b][k]|, complex moduli)
---------------------------------------------------------------------------------
    tol_pred = C_PRED (2n + 4) u S_p,      C_PRED = 4.
The kernel runs the 3M form on the f64 matrix cores: three real dot products of length n,
P1 = sum xr cr, P2 = sum xi ci, P3 = sum fl(xr + xi) fl(cr + ci), then Re = fl(P1 - P2), Im = fl(fl(P3 - P1) - P2).
Whatever the order inside an MFMA, a length-n dot product is within gamma_n = n u / (1 - n u) of its absolute
sum (Higham, Accuracy and Stability, (3.5)).  With |xr cr| + |xi ci| <= |x| |c| (Cauchy-Schwarz) and
|xr + xi| |cr + ci| <= 2 |x| |c|, to first order in u:
    |dRe| <= gamma_n S + u |Re|                          <= (n + 1) u S
    |dIm| <= (gamma_n + 2u) 2S + gamma_n S + 2u (3S)     <= 3 (n + 4) u S   (pre-additions: one rounding per factor;
                                                            two subtractions on partial results of at most 3S)
so the complex error is at most sqrt(1 + 9) (n + 4) u S = 3.17 (n + 4) u S, the modulus moves by no more than
that, and hypot adds its own rounding, taken as 2 ulp = 4u |z| <= 4u S.  Total (3.17 (n + 4) + 4) u S; against
(2n + 4) u S that is a factor 3.31 at n = 1, 2.88 at n = 2 and falls to 1.59 as n grows: C_PRED = 4 covers every
n >= 1 with room for the second-order terms (n u < 2^-40 here).  The numpy restatement (a 4M zgemm, at most
gamma_2n sqrt(2) S) lies inside the same bound.

Propagation to the statistics (N = n_used, rel the exact values)
----------------------------------------------------------------
    d_p      = tol_pred_p / rss_p + 2u rel_p                  (the subtraction and the division)
    tol_mean = sum d_p / N + (N + 1) u mean                   (N - 1 additions in any order, one division)
    tol_ms   = sum (2 rel_p d_p + d_p^2) / N + (N + 2) u ms   (the squares, the sum, the division)
    tol_rms  = tol_ms / rms + 2u rms                          (|sqrt a - sqrt b| <= |a - b| / sqrt b; sqrt(tol_ms) if rms = 0)
    tol_max  = max d_p                                        (|max a - max b| <= max |a - b|)
n_used, the status word and the values of a degenerate realisation (1, 1, 1, 0) are compared exactly.
"""
import functools
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import linop_ref as LR  # noqa: E402

U = 2.0 ** -53
C_PRED = 4.0
ST_DEGENERATE, ST_SKIPPED = 256, 512

# (batch, n, Pt) of the GPU parity suite: K-loop tail (n not a multiple of 4, of 16), masked row and realisation
# tiles, a single tile, several Pt tiles per work-group (Pt > 128) and several work-groups (batch > 16)
SHAPES = [(1, 1, 1), (1, 16, 1), (3, 9, 5), (17, 64, 33), (16, 256, 16), (5, 1024, 70), (33, 144, 257),
          (64, 256, 1200)]
KINDS = ("random", "phase")


def _rss2d(rss, batch):
    rss = np.asarray(rss, np.float64)
    return np.broadcast_to(rss, (batch, rss.shape[-1])) if rss.ndim == 1 else rss


def _stats(rel, usable, bad, xp=np.float64):
    """metrics [batch][4] and status [batch] from rel [batch][Pt] under the library's rules."""
    batch = rel.shape[0]
    met = np.ones((batch, 4), xp)
    met[:, 3] = 0
    st = np.zeros(batch, np.uint32)
    for b in range(batch):
        if not usable[b].all():
            st[b] |= ST_SKIPPED
        r = rel[b][usable[b]]
        N = r.size
        if bad[b] or N == 0:
            st[b] |= ST_DEGENERATE
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            vals = (r.sum() / N, np.sqrt((r * r).sum() / N), r.max())
        if not all(np.isfinite(v) for v in vals):
            st[b] |= ST_DEGENERATE
            continue
        met[b] = (*vals, N)
    return met, st


def evaluate_rss(X, CB, rss, model=None):
    """numpy f64 restatement: (metrics [batch][4], status [batch], pred [batch][Pt]).  ``model``: one of the
    deliberately wrong variants "conj", "square", "div_pt", "diff_first" (tests/test_rss_ref.py)."""
    X = np.atleast_2d(np.asarray(X, np.complex128))
    CB = np.atleast_2d(np.asarray(CB, np.complex128))
    batch = X.shape[0]
    rss = _rss2d(rss, batch)
    usable = np.isfinite(rss) & (rss > 0)
    bad = ~np.isfinite(X.view(np.float64)).all(axis=1)
    with np.errstate(all="ignore"):
        z = X @ (CB.conj() if model == "conj" else CB).T
        pred = np.abs(z)
        if model == "square":
            pred = pred * pred
        rel = (np.abs(z - rss) if model == "diff_first" else np.abs(pred - rss)) / rss
    met, st = _stats(rel, usable, bad)
    if model == "div_pt":
        live = (st & ST_DEGENERATE) == 0
        N, Pt = met[live, 3], rss.shape[1]
        met[live, 0] *= N / Pt
        met[live, 1] *= np.sqrt(N / Pt)
    return met, st, pred


def exact(X, CB, rss):
    """Exact reference and tolerances: a dict with ``metrics`` [batch][4] and ``pred`` [batch][Pt] (longdouble),
    ``status``, ``tol_pred`` [batch][Pt] and ``tol`` [batch][3] (mean, rms, max; f64).  X must be finite."""
    X = np.atleast_2d(np.asarray(X, np.complex128))
    CB = np.atleast_2d(np.asarray(CB, np.complex128))
    batch, n = X.shape
    rss = _rss2d(rss, batch)
    hi, lo = LR.exact_cmatvec(CB, X)
    ld = np.longdouble
    re = hi[:, 0::2].astype(ld) + lo[:, 0::2].astype(ld)
    im = hi[:, 1::2].astype(ld) + lo[:, 1::2].astype(ld)
    pred = np.hypot(re, im)
    usable = np.isfinite(rss) & (rss > 0)
    with np.errstate(all="ignore"):
        rel = np.abs(pred - rss.astype(ld)) / rss.astype(ld)
    met, st = _stats(rel, usable, np.zeros(batch, bool), ld)
    S = np.abs(X) @ np.abs(CB).T
    tol_pred = C_PRED * (2 * n + 4) * U * S
    tol = np.zeros((batch, 3))
    for b in range(batch):
        if st[b] & ST_DEGENERATE:
            continue
        u_ = usable[b]
        r = rel[b][u_].astype(np.float64)
        N = r.size
        d = tol_pred[b][u_] / rss[b][u_] + 2 * U * r
        mean, rms = float(met[b, 0]), float(met[b, 1])
        tol_ms = np.sum(2 * r * d + d * d) / N + (N + 2) * U * rms * rms
        tol[b] = (d.sum() / N + (N + 1) * U * mean,
                  (tol_ms / rms if rms > 0 else np.sqrt(tol_ms)) + 2 * U * rms,
                  d.max())
    return {"metrics": met, "status": st, "pred": pred, "tol_pred": tol_pred, "tol": tol}


def ratios(met, pred, ref):
    """Worst err / tol of pred (None: not compared) and of the three statistics against ``exact``'s dict, over
    the non-degenerate realisations; n_used and the rest are the caller's exact comparisons."""
    ld = np.longdouble
    live = (ref["status"] & ST_DEGENERATE) == 0
    out = {}
    if pred is not None:
        e = np.abs(np.asarray(pred, np.float64).astype(ld) - ref["pred"]).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(e == 0, 0.0, e / ref["tol_pred"])
        out["pred"] = float(np.max(q)) if q.size else 0.0
    e = np.abs(np.asarray(met, np.float64)[:, :3].astype(ld) - ref["metrics"][:, :3]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(e == 0, 0.0, e / ref["tol"])[live]
    for i, name in enumerate(("mean", "rms", "max")):
        out[name] = float(np.max(q[:, i])) if q.size else 0.0
    return out


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def codebook(rng, kind, Pt, n):
    """"random": complex normals with full mantissas; "phase": c (+-1, +-j) with c = 1 / sqrt(n)."""
    if kind == "random":
        return rng.standard_normal((Pt, n)) + 1j * rng.standard_normal((Pt, n))
    return (1j ** rng.integers(0, 4, (Pt, n))) * (1.0 / np.sqrt(n))


@functools.lru_cache(maxsize=None)
def case(batch, n, Pt, kind):
    """Seeded inputs of one parity case, with their exact reference (computed once, shared, read-only): X with a
    per-realisation scale over 2^+-8, rss [batch][Pt] = |CB x| e^{0.3 g} (relative errors of a few tenths), except
    every fourth realisation, whose rss is |CB x| (1 + 1e-9 g): the cancellation in pred - rss."""
    rng = np.random.default_rng([batch, n, Pt, KINDS.index(kind)])
    CB = codebook(rng, kind, Pt, n)
    X = (rng.standard_normal((batch, n)) + 1j * rng.standard_normal((batch, n))) * np.exp2(rng.uniform(-8, 8, (batch, 1)))
    g = rng.standard_normal((batch, Pt))
    fac = np.exp(0.3 * g)
    fac[3::4] = 1 + 1e-9 * g[3::4]
    rss = np.abs(X @ CB.T) * fac
    rss[rss <= 0] = 1.0
    ref = exact(X, CB, rss)
    _freeze(X, CB, rss, *(v for v in ref.values()))
    return {"X": X, "CB": CB, "rss": rss, "ref": ref}


@functools.lru_cache(maxsize=None)
def skip_case():
    """The skip and degenerate rules at (batch, n, Pt) = (12, 64, 33): rows with rss of 0, a negative value, NaN
    and Inf (realisations 1-4, and all four kinds together in 5), an all-skipped realisation (6), an X with one
    NaN (7), one Inf (8), an all-zero X (9); 0, 10, 11 are plain.  ``plain`` holds the same inputs with finite
    positive rss and finite X, for the neighbours' bit-for-bit comparison."""
    c = case(17, 64, 33, "random")
    X, CB, rss = c["X"][:12].copy(), c["CB"], c["rss"][:12].copy()
    plain = {"X": X.copy(), "rss": rss.copy()}
    for b, v in ((1, 0.0), (2, -1.5), (3, np.nan), (4, np.inf)):
        rss[b, [2, 17 + b]] = v
    rss[5, [0, 5, 20, 32]] = (0.0, -2.0, np.nan, np.inf)
    rss[6] = np.resize([0.0, -1.0, np.nan, -np.inf], 33)
    X[7, 13] = complex(np.nan, 1.0)
    X[8, 63] = complex(0.5, np.inf)
    X[9] = 0
    Xf = X.copy()
    Xf[[7, 8]] = plain["X"][[7, 8]]          # exact() takes finite X; 7 and 8 are degenerate by rule
    ref = exact(Xf, CB, rss)
    ref["status"] = ref["status"].copy()
    ref["status"][[7, 8]] |= ST_DEGENERATE
    for k in ("metrics", "tol"):
        ref[k] = ref[k].copy()
    ref["metrics"][[7, 8]] = (1, 1, 1, 0)
    ref["tol"][[7, 8]] = 0
    _freeze(X, rss, plain["X"], plain["rss"], *(v for v in ref.values()))
    return {"X": X, "CB": CB, "rss": rss, "ref": ref, "plain": plain,
            "degenerate": [6, 7, 8], "skipped": [1, 2, 3, 4, 5, 6], "zero": 9, "plain_rows": [0, 10, 11]}
