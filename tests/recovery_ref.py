"""numpy restatement of the reference's score for sparse recoveries, for the recovery evaluator's tests.

  Evaluation_Recovery   Numerical_Simulation/src/evaluate_plot_results/Evaluation_Recovery.m:73-338
  MyBeamSweeping        Numerical_Simulation/src/evaluate_plot_results/MyBeamSweeping.m:119-157 (the read-out only)
  Quantize_PS           Numerical_Simulation/src/generate_sensing_matrix/Quantize_PS.m:61-73 (eval_ref.quantize_ps)

One realisation at a time, in float64 with numpy.linalg.svd in eval_ref's gauge.  Written from the behaviour of the
reference, quirks included (each cites its line):

  * :86-88   the L entries of z largest in modulus (an exact tie to the lower index: the build's stated departure
             from MATLAB's tie-break by phase angle), then in ascending index order;
  * :127-132 the true AoD sorted descending; :128 assigns AoA_True(order) = AoA_True(order), which changes nothing,
             so the true AoA keep their order; the estimates ordered by estimated AoD descending, AoA following;
  * :149-161 the quantisation error for L == 1 only;
  * :194     Num_RFchains = 1: every beam through Quantize_PS;
  * :226-227 the "AoDA" beams at index l left over from :169's loop: the last sorted estimate;
  * :277-282 eye(L) + scalar adds the scalar to every entry: det = 1 + L |g|^2 / sigma^2;
  * :289-317 columns 12-14 are Evaluation_H of (H_est, H).

AD z is evaluated through AD's Kronecker structure, A_r^T mat(z)^T conj(A_t) (tests/test_recovery_ref.py checks it
against the dense product with sparse.dictionary_2d).  The sweep is not redone: the two patterns' picks come in, as
the build's entry takes them.
"""
import numpy as np

import eval_ref

NCOL = 15
QUANTISED = (5, 6, 7, 8, 9, 12)   # zero-based columns that go through Quantize_PS


def steer(n, deg, kappa):
    """exp(-1i*2*pi/lambda*d*sind(deg).*(0:n-1)).'/sqrt(n) (:170-173)."""
    ph = kappa * np.sin(np.deg2rad(deg)) * np.arange(n)
    return (np.cos(ph) - 1j * np.sin(ph)) / np.sqrt(n)


def channel_from_z(z, tb):
    """AD z as the rx x tx matrix (entry (r, t) = vec[r + rx t]), through the Kronecker structure."""
    Z = np.asarray(z, np.complex128).reshape(tb.Qt, tb.Qr)
    return tb.A_r.T @ Z.T @ np.conj(tb.A_t)


def vec(M):
    """Column-major vectorisation: entry r + rx t."""
    return M.T.reshape(-1)


def picks_of(z, L):
    """:86-88, zero-based."""
    return np.sort(np.argsort(-np.abs(z), kind="stable")[:L])


def rate(g, L, noise_power):
    return abs(np.log2(1.0 + L * abs(g) ** 2 / noise_power))


def _err(tx, rx, ed, ea):
    return ea if tx == 1 else ed if rx == 1 else (ed + ea) / 2.0


def evaluation_recovery(z, vecH, aod_deg, aoa_deg, tb, true_idx, noise_power, picks=None, sweep=None, tol=1e-6):
    """(metrics [15], H_est [tx*rx], near_boundary) of one realisation.  ``tb``: the per-call tables (A_t [Qt][tx],
    A_r [Qr][rx], deg_t, deg_r, first_t, first_r, kappa, tx, rx); ``true_idx`` [L][2] zero-based global grid indices;
    ``picks`` [2][2] zero-based (ind_F, ind_W) of pattern 1 and 2 with ``sweep`` (centre_deg_*, peak_deg_*).
    near_boundary: an entry of a vector that is quantised lies within ``tol`` rad of a quantisation boundary."""
    z = np.asarray(z, np.complex128).reshape(-1)
    h = np.asarray(vecH, np.complex128).reshape(-1)
    aod, aoa = np.asarray(aod_deg, np.float64).reshape(-1), np.asarray(aoa_deg, np.float64).reshape(-1)
    tx, rx, L, kap = tb.tx, tb.rx, len(aod), tb.kappa
    out = np.full(NCOL, np.nan)
    # :86-124
    pk = picks_of(z, L)
    pu, pv = pk // tb.Qr, pk % tb.Qr
    eD, eA = tb.deg_t[pu], tb.deg_r[pv]
    # :127-132
    tD = aod[np.argsort(-aod, kind="stable")]
    tA = aoa   # (:128)
    oe = np.argsort(-eD, kind="stable")
    eD, eA = eD[oe], eA[oe]
    # :135-146
    out[1] = _err(tx, rx, np.mean(np.abs(eD - tD)), np.mean(np.abs(eA - tA)))
    # :149-161
    if L == 1:
        qd = abs(int(true_idx[0][0]) - (tb.first_t + int(pu[0])))
        qa = abs(int(true_idx[0][1]) - (tb.first_r + int(pv[0])))
        out[0] = _err(tx, rx, qd, qa)
    else:
        out[0] = 0.0
    # :165-183
    mt = sum(np.linalg.norm(steer(tx, tD[l], kap) - steer(tx, eD[l], kap)) ** 2 for l in range(L)) / \
        sum(np.linalg.norm(steer(tx, tD[l], kap)) ** 2 for l in range(L))
    mr = sum(np.linalg.norm(steer(rx, tA[l], kap) - steer(rx, eA[l], kap)) ** 2 for l in range(L)) / \
        sum(np.linalg.norm(steer(rx, tA[l], kap)) ** 2 for l in range(L))
    out[2] = _err(tx, rx, mt, mr)
    # :187-191
    he = vec(channel_from_z(z, tb))
    he = he * np.exp(1j * np.angle(np.vdot(he, h) / np.vdot(h, h)))
    out[3] = np.linalg.norm(he - h) ** 2 / np.linalg.norm(h) ** 2
    # :196-203, :268-269, :277-278
    G, E = eval_ref.mat(h, rx, tx), eval_ref.mat(he, rx, tx)
    ug, vg = eval_ref.top_vectors(G)
    margins = [eval_ref.boundary_margin(ug), eval_ref.boundary_margin(vg)]
    out[4] = rate(np.linalg.svd(G, compute_uv=False)[0], L, noise_power)
    out[5] = rate(np.vdot(eval_ref.quantize_ps(ug), G @ eval_ref.quantize_ps(vg)), L, noise_power)
    # :212-217, :270, :279 and :289-317
    _, gain_ana, gain_dig, proj = eval_ref.evaluation_h(he, h, rx, tx)
    u1, v1 = eval_ref.top_vectors(E)
    margins += [eval_ref.boundary_margin(u1), eval_ref.boundary_margin(v1)]
    out[6] = rate(gain_ana, L, noise_power)
    out[12], out[13], out[14] = gain_ana, gain_dig, proj
    # :226-229, :271, :280
    f, w = steer(tx, eD[L - 1], kap), steer(rx, eA[L - 1], kap)
    margins += [eval_ref.boundary_margin(f), eval_ref.boundary_margin(w)]
    out[7] = rate(np.vdot(eval_ref.quantize_ps(w), G @ eval_ref.quantize_ps(f)), L, noise_power)
    # :232-259, :272-273, :281-282
    if picks is not None:
        for pat, est_t, est_r in ((0, sweep.peak_deg_t, sweep.peak_deg_r), (1, sweep.centre_deg_t, sweep.centre_deg_r)):
            iF, iW = int(picks[pat][0]), int(picks[pat][1])
            f, w = steer(tx, sweep.centre_deg_t[iF], kap), steer(rx, sweep.centre_deg_r[iW], kap)
            margins += [eval_ref.boundary_margin(f), eval_ref.boundary_margin(w)]
            out[8 + pat] = rate(np.vdot(eval_ref.quantize_ps(w), G @ eval_ref.quantize_ps(f)), L, noise_power)
            out[10 + pat] = _err(tx, rx, np.mean(np.abs(est_t[iF] - tD)), np.mean(np.abs(est_r[iW] - tA)))
    return out, he, min(margins) < tol


def evaluate(Z, H, aod, aoa, tb, true_idx, noise_power, picks=None, sweep=None):
    """[batch][15] metrics, [batch][tx*rx] H_est and the [batch] near-boundary mask."""
    res = [evaluation_recovery(Z[b], H[b], aod[b], aoa[b], tb, true_idx[b], noise_power,
                               None if picks is None else picks[b], sweep) for b in range(len(Z))]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], dtype=bool))


def gains_of(metrics_row, L, noise_power):
    """|g| behind a rate: the inverse of ``rate`` on its increasing branch."""
    return np.sqrt(np.maximum(2.0 ** metrics_row - 1.0, 0.0) * noise_power / L)


def peak_angles(beams, kappa, grid):
    """MyBeamSweeping.m:134-154: (the first angle of ``grid`` maximising |f^H a(theta)|, the gains [M][len(grid)])."""
    beams = np.atleast_2d(np.asarray(beams, np.complex128))
    n = beams.shape[1]
    ph = kappa * np.sin(np.deg2rad(grid))[:, None] * np.arange(n)[None, :]
    a = np.cos(ph) - 1j * np.sin(ph)                      # [angle][antenna]
    gain = np.abs(np.conj(beams) @ a.T)                   # [M][angle]
    return grid[np.argmax(gain, axis=1)], gain


def seeded_problem(seed, batch, tb, L, search_deg, noise=0.05):
    """Parity inputs on the tables ``tb``: per realisation L paths at off-grid angles inside the searching area with
    unit-norm CN gains (H = sqrt(tx rx) sum g a_r a_t^H) plus 2 % of diffuse channel; and z of three kinds by
    b % 3: 0 dense (the on-grid truth plus CN noise on every entry, like GAMP's output), 1 L-sparse with exact zeros
    (the truth's nearest atoms shifted by up to one index, like OMP's; atoms may coincide, which leaves exact ties at
    zero), 2 the largest entries in the last and in the first atom of the cut grid over a small dense floor.
    Returns (Z, H, aod_deg, aoa_deg, true_idx)."""
    rng = np.random.default_rng(seed)
    tx, rx, Qt, Qr = tb.tx, tb.rx, tb.Qt, tb.Qr
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)  # noqa: E731
    half = 0.5 * min(search_deg, 178.0)
    aod = rng.uniform(-half, half, (batch, L))
    aoa = rng.uniform(-half, half, (batch, L))
    g = cn(batch, L)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    tidx = tb.true_indices(aod, aoa)
    H = np.zeros((batch, tx * rx), np.complex128)
    Z = np.zeros((batch, Qt * Qr), np.complex128)
    sc = np.sqrt(tx * rx)
    for b in range(batch):
        M = sum(g[b, l] * sc * np.outer(steer(rx, aoa[b, l], tb.kappa), np.conj(steer(tx, aod[b, l], tb.kappa)))
                for l in range(L))
        H[b] = vec(M) + 0.02 * cn(tx * rx)
        cu = np.clip(tidx[b, :, 0] - tb.first_t, 0, Qt - 1)
        cv = np.clip(tidx[b, :, 1] - tb.first_r, 0, Qr - 1)
        kind = b % 3
        if kind == 0:
            Z[b] = noise * sc / np.sqrt(Qt * Qr) * cn(Qt * Qr)
            for l in range(L):
                Z[b, cu[l] * Qr + cv[l]] += g[b, l] * sc
        elif kind == 1:
            for l in range(L):
                u = int(np.clip(cu[l] + rng.integers(-1, 2), 0, Qt - 1))
                v = int(np.clip(cv[l] + rng.integers(-1, 2), 0, Qr - 1))
                Z[b, u * Qr + v] = g[b, l] * sc * (1.0 + 0.1 * rng.standard_normal())
        else:
            Z[b] = 1e-3 * sc / np.sqrt(Qt * Qr) * cn(Qt * Qr)
            big, small = (Qt * Qr - 1, 0) if (b // 3) % 2 == 0 else (0, Qt * Qr - 1)
            Z[b, big] = sc * np.exp(2j * np.pi * rng.random())
            if Qt * Qr > 1:
                Z[b, small] = 0.7 * sc * np.exp(2j * np.pi * rng.random())
    return Z, H, aod, aoa, tidx
