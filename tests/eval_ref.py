"""numpy restatement of the reference's channel score, for the evaluator's tests.

  Evaluation_H   Numerical_Simulation/src/evaluate_plot_results/Evaluation_H.m:73-132
  Quantize_PS    Numerical_Simulation/src/generate_sensing_matrix/Quantize_PS.m:61-73

One realisation at a time, in float64 with numpy.linalg.svd (zgesdd).  MATLAB's svd leaves the unit
phase of a singular pair unpinned, and gain_ana quantises those phases; the gauge used here is the one
the build's beamformer reproduces and tests: v1 = conj(row 0 of Vh of svd(E)), u1 = row 0 of Vh of
svd(E^T), with E = mat(x) the tx x rx matrix of entries x[i + tx*j].
"""
import numpy as np

# phi_qua = -pi:2*pi/Nps:pi at Phase_Bit = 2 (Quantize_PS.m:63-64)
PHI_QUA = np.array([-np.pi, -np.pi / 2, 0.0, np.pi / 2, np.pi])


def mat(v, tx, rx):
    """tx x rx matrix with entry (i, j) = v[i + tx*j] (include/ace.h's vec(H) order)."""
    return np.asarray(v, dtype=np.complex128).reshape(rx, tx).T


def quantize_ps(v):
    """Quantize_PS.m:61-73 for a vector at 2 bits: the first nearest grid phase (:69), unit modulus over
    sqrt(len) (:70)."""
    v = np.asarray(v, dtype=np.complex128)
    ind = np.argmin(np.abs(np.angle(v)[:, None] - PHI_QUA[None, :]), axis=1)
    return np.exp(1j * PHI_QUA[ind]) / np.sqrt(len(v))


def top_vectors(E):
    """(u1, v1) of E in the stated gauge."""
    v1 = np.conj(np.linalg.svd(E)[2][0])
    u1 = np.linalg.svd(E.T)[2][0]
    return u1, v1


def boundary_margin(v):
    """Smallest distance (rad) of an entry's phase to a quantisation boundary (the odd multiples of pi/4)."""
    r = np.mod(np.angle(v) - np.pi / 4, np.pi / 2)
    return float(np.min(np.minimum(r, np.pi / 2 - r)))


def rank_one_part(M):
    """U(:,1)*S(1,1)*V(:,1)' vectorised column-major (Evaluation_H.m:107-113)."""
    U, S, Vh = np.linalg.svd(M)
    return (S[0] * np.outer(U[:, 0], Vh[0])).T.reshape(-1)


def evaluation_h(x, g, tx, rx):
    """(nmse, gain_ana, gain_dig, proj_err) of the estimate x against the truth g."""
    x = np.asarray(x, dtype=np.complex128).reshape(-1)
    g = np.asarray(g, dtype=np.complex128).reshape(-1)
    E, G = mat(x, tx, rx), mat(g, tx, rx)
    # :87-89 (the value of :85 is overwritten)
    nmse = np.linalg.norm(g - np.vdot(x, g) / np.vdot(x, x) * x) ** 2 / np.linalg.norm(g) ** 2
    # :95-104
    u1, v1 = top_vectors(E)
    w_q, f_q = quantize_ps(u1), quantize_ps(v1)
    w_dig, f_dig = u1 / np.linalg.norm(u1), v1 / np.linalg.norm(v1)
    gain_ana = abs(np.vdot(w_q, G @ f_q))
    gain_dig = abs(np.vdot(w_dig, G @ f_dig))
    # :107-115
    X_gt, X = rank_one_part(G), rank_one_part(E)
    proj_err = np.linalg.norm(X_gt - np.vdot(X, X_gt) / np.vdot(X, X) * X) / np.linalg.norm(X_gt)
    return float(nmse), float(gain_ana), float(gain_dig), float(proj_err)


def near_boundary(x, tx, rx, tol=1e-6):
    """True when an entry of u1 or v1 lies within tol rad of a quantisation boundary: a rounding-level phase
    difference between two correct SVDs may then flip a 2-bit code, and gain_ana with it."""
    u1, v1 = top_vectors(mat(x, tx, rx))
    return min(boundary_margin(u1), boundary_margin(v1)) < tol


def evaluate(X, G, tx, rx):
    """[batch][4] metrics and the [batch] near-boundary mask."""
    met = np.array([evaluation_h(x, g, tx, rx) for x, g in zip(X, G)]).reshape(-1, 4)
    nb = np.array([near_boundary(x, tx, rx) for x in X], dtype=bool)
    return met, nb


def seeded_problem(seed, batch, tx, rx):
    """Parity inputs: G a 3-path sum of outer products of unit-modulus vectors (path gains 1, 1/2, 1/4 with
    random phases: sigma1 - sigma2 stays well away from zero) plus 1e-2 noise, entries O(1);
    x = e^{j theta} (G + delta noise), delta per realisation from {1e-4, 1e-2, 0.3}: nmse and proj_err span
    1e-8 .. 1e-1."""
    rng = np.random.default_rng(seed)
    n = tx * rx
    cn = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)  # noqa: E731
    G = np.zeros((batch, n), np.complex128)
    for l, amp in enumerate((1.0, 0.5, 0.25)):
        a = np.exp(2j * np.pi * rng.random((batch, tx)))
        b = np.exp(2j * np.pi * rng.random((batch, rx)))
        gain = amp * np.exp(2j * np.pi * rng.random((batch, 1, 1)))
        # entry (i, j) at i + tx*j: [batch][rx][tx] row-major
        G += (gain * b[:, :, None] * a[:, None, :]).reshape(batch, n)
    G += 1e-2 * cn(batch, n)
    delta = rng.choice([1e-4, 1e-2, 0.3], size=(batch, 1))
    theta = 2 * np.pi * rng.random((batch, 1))
    X = np.exp(1j * theta) * (G + delta * cn(batch, n))
    return X, G
