"""The four linear operators of the ADMM iteration on their own, against exact references (tests/linop_ref.py):

    T = (Y - M/mu) - A (Z - N/mu)      X = (Z - N/mu) + A^H g      KY = K Y      g = G T

through the test entry ace_linop_host (ace_amd.linops), which builds the operators with the solver's setup and
makes the launcher calls a solve makes, on every path: f64 3M matrix-core GEMM (pre-pass + GEMM, and the GEMM
with the pre-pass folded in), f64 GEMV (private codebooks), exact int8 digit planes (unit path and the r-column
stages); and the GEMM launcher with all of its arguments (ace_zgemm_host).

Recipes: 1 integer data, bit-exact; 2 full-mantissa data within the derived tolerances; 3 exponent edges of the
digit planes; 4 isolation of a non-finite vector and the done / nzero / avok flags; 5 position invariance;
6 int8 against f64.  Every tolerance comes from linop_ref (derived there from the kernels' arithmetic); the
printed ratios are max(err / tol) per operator and path.
"""
import pathlib

import numpy as np
import pytest

import linop_ref as R

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]

# (m, n, batch, codebook kind): the sizes cross the K stages of 32 complex, the 64-complex staging blocks, the g
# re-read past 256 entries, the 256- / 512-real output blocks, 16 vectors per work-group and the GEMM tiles
SHAPES = [
    (1, 1, 1, "pmj1"),
    (15, 33, 37, "pmj1"),
    (257, 64, 17, "synth"),      # second 512-real output block of apply_A
    (300, 100, 17, "off"),       # g re-read past 256 in apply_AH / apply_K, ragged K
    (121, 1024, 16, "twin"),     # four output blocks of apply_AH, K_int = 2n
    (1, 31, 15, "pmj"),
    (15, 32, 16, "synth"),
    (121, 65, 1, "pmj"),
    (256, 257, 15, "off"),
    (15, 1, 17, "pmj1"),
    (256, 64, 37, "pmj"),
    (121, 31, 17, "synth"),
]
IDS = [f"m{m}-n{n}-b{b}-{k}" for m, n, b, k in SHAPES]
PRIVATE_MAX = 300 * 100 * 17   # private codebooks (one A per realisation) at the shapes up to this many entries


def _lin():
    from ace_amd import linops
    return linops


def _check(err, tol, label, floor=0.0):
    """Assert err <= tol everywhere; print and return max(err / tol)."""
    t = np.maximum(tol, floor)
    bad = err > t
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(t > 0, err / t, np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"  {label}: max err/tol {worst:.3g}")
    if bad.any():
        j, i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{label}: vector {j}, real output {i}: err {err[j, i]:.3e} > tol {t[j, i]:.3e} "
                             f"({int(bad.sum())} of {bad.size} outputs outside)")
    return worst


def _same(a, b, label):
    """Bit-for-bit equality of two complex arrays, NaN patterns included (only +0 and -0 count as equal)."""
    af, bf = np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)
    assert af.shape == bf.shape, (label, af.shape, bf.shape)
    ne = (af.view(np.uint64) != bf.view(np.uint64)) & ~((af == 0.0) & (bf == 0.0))
    if ne.any():
        j, i = np.argwhere(ne)[0]
        raise AssertionError(f"{label}: differs first at vector {j}, real output {i}: {af[j, i]!r} vs {bf[j, i]!r} "
                             f"({int(ne.sum())} of {ne.size} components differ)")


class Problem:
    """One codebook with its integer parts and exact operators."""

    def __init__(self, m, n, kind, unit=False, seed=0):
        A = R.codebook(kind, m, n, seed)
        c, P, Q = R.phase_parts(A)
        if unit:
            c, A = 1.0, (P + 1j * Q).astype(np.complex128)
        self.m, self.n, self.A, self.c = m, n, A, c
        self.c2 = c * c   # (the setup forms c^2 as this f64 product)
        self.G = P + 1j * Q
        self.EA = R.real_expand(self.G)
        self.EH = R.real_expand(self.G.conj().T)
        Kr, Ki = R.kint(A)
        self.Kint = Kr + 1j * Ki
        self.EK = R.real_expand(self.Kint)


def _vb(V, batch):
    """Per-realisation bound max|V| (as the Z-step would leave it)."""
    return R.maxabs_rows(V).reshape(batch, -1).max(axis=1)


def _mu_imu(rng, batch, rcols=1, pow2=False):
    mu = np.exp2(rng.integers(0, 3, batch).astype(np.float64)) if pow2 else rng.uniform(0.5, 4.0, batch)
    return mu, R.per_vector(1.0 / mu, batch * rcols, rcols)


# ------------------------------------------------------------------------------------------ recipe 1
@pytest.mark.parametrize("m,n,batch,kind", SHAPES, ids=IDS)
def test_integer_data_is_bit_exact(gpu, m, n, batch, kind):
    """c = 1 and integer data below 2^20 with mu a power of two: every f64 and digit-plane operation is exact,
    so each operator on each path equals the int64 numpy product bit for bit (any wrong index, tail, stride,
    mode, conjugation or sign fails), and K of the setup is the integer (P + jQ)(P + jQ)^H."""
    L = _lin()
    rng = np.random.default_rng([1, m, n, batch])
    pb = Problem(m, n, kind, unit=True)
    mu, imu = _mu_imu(rng, batch, pow2=True)
    Z, Y, g = R.int_vectors(rng, batch, n, 19), R.int_vectors(rng, batch, m, 19), R.int_vectors(rng, batch, m, 20)
    N = R.int_vectors(rng, batch, n, 19) * mu[:, None]
    M = R.int_vectors(rng, batch, m, 19) * mu[:, None]
    V, S = Z - N * imu[:, None], Y - M * imu[:, None]   # exact

    def iprod(E, X):
        return (X.view(np.float64).astype(np.int64) @ E.astype(np.int64).T).astype(np.float64).view(np.complex128)
    T_ref, W_ref, KY_ref = S - iprod(pb.EA, V), iprod(pb.EH, g), iprod(pb.EK, g)
    X_ref = V + W_ref
    K, _, c = L.linop_host("setup", "i8", pb.A)
    assert np.array_equal(K, pb.Kint) and c[0] == 1.0 and c[1] == 1.0
    if kind == "twin":
        assert K[0, 1] == 2 * n
    kw = dict(mu=mu, vbound=_vb(V, batch))
    for path in ("f64", "f64_fused", "i8"):
        _same(L.linop_host("A", path, pb.A, Z=Z, N=N, Y=Y, M=M, **kw), T_ref, f"A {path}")
        out = L.linop_host("AH", path, pb.A, Z=Z, N=N, g=g, **kw)
        _same(out, W_ref if path == "i8" else X_ref, f"AH {path}")
    for path in ("f64", "i8"):
        _same(L.linop_host("K", path, pb.A, g=g, **kw), KY_ref, f"K {path}")
    if m * n * batch <= PRIVATE_MAX:   # private codebooks: two different codes, alternating
        pb2 = Problem(m, n, "pmj1", unit=True, seed=1)
        Ap = np.stack([(pb, pb2)[b % 2].A for b in range(batch)])
        odd = (np.arange(batch) % 2 == 1)[:, None]
        _same(L.linop_host("A", "f64", Ap, Z=Z, N=N, Y=Y, M=M, **kw),
              np.where(odd, S - iprod(pb2.EA, V), T_ref), "A private")
        _same(L.linop_host("AH", "f64", Ap, Z=Z, N=N, g=g, **kw),
              np.where(odd, V + iprod(pb2.EH, g), X_ref), "AH private")
        _same(L.linop_host("K", "f64", Ap, g=g, **kw), np.where(odd, iprod(pb2.EK, g), KY_ref), "K private")
        Kp, _, _ = L.linop_host("setup", "f64", Ap)
        assert np.array_equal(Kp[0], pb.Kint) and (batch < 2 or np.array_equal(Kp[1], pb2.Kint))


# ------------------------------------------------------------------------------------------ recipes 2 and 6
def _refs(pb, Z, N, Y, M, g, imu):
    """Exact references of one problem's operators on full-mantissa data."""
    r = {}
    r["V"], r["S"] = R.fma_ref(N, imu, Z), R.fma_ref(M, imu, Y)
    r["AV"] = R.exact_matvec(pb.EA, r["V"].view(np.float64), pb.c)
    r["W"] = R.exact_matvec(pb.EH, g.view(np.float64), pb.c)
    r["KY"] = R.exact_matvec(pb.EK, g.view(np.float64), pb.c2)
    r["T"] = (r["S"].view(np.float64) - r["AV"][0]).view(np.complex128)
    r["X"] = (r["V"].view(np.float64) + r["W"][0]).view(np.complex128)
    return r


def _tols(pb, r, N, M, g, imu, eV):
    """Derived tolerances per operator: int8 (exponent eV for apply_A, the pre-pass maximum for A^H / K) and f64."""
    eg = R.kernel_exp(R.maxabs_rows(g))
    t = {}
    t["A", "i8"] = R.i8_tol(pb.EA, pb.c, eV, r["AV"][0], S=r["S"], T=r["T"])
    t["A", "f64"] = (R.gemm_tol(pb.A, r["V"], E=r["S"], C=r["T"]) + R.pre_rounding(pb.A, N, imu)
                     + R.own_rounding(M, imu))
    t["W", "i8"] = R.i8_tol(pb.EH, pb.c, eg, r["W"][0])
    t["X", "i8"] = R.i8_tol(pb.EH, pb.c, eg, r["W"][0], S=r["V"], T=r["X"])
    t["X", "f64"] = R.gemm_tol(pb.A, g, E=r["V"], C=r["X"], herm=True) + R.own_rounding(N, imu)
    t["K", "i8"] = R.i8_tol(pb.EK, pb.c2, eg, r["KY"][0])
    return t


@pytest.mark.parametrize("m,n,batch,kind", SHAPES, ids=IDS)
def test_random_data_within_derived_tolerance(gpu, m, n, batch, kind):
    """Full-mantissa data: every output within the derived tolerance of the exact reference (recipe 2), and the
    int8 and f64 results within the sum of their tolerances of each other (recipe 6).  K of the setup is within the
    GEMM tolerance of c^2 K_int, and the f64 K Y within the GEMM tolerance of the exact product with that K."""
    L = _lin()
    rng = np.random.default_rng([2, m, n, batch])
    pb = Problem(m, n, kind)
    mu, imu = _mu_imu(rng, batch)
    Z, N = R.rand_vectors(rng, batch, n), R.rand_vectors(rng, batch, n)
    Y, M, g = R.rand_vectors(rng, batch, m), R.rand_vectors(rng, batch, m), R.rand_vectors(rng, batch, m)
    r = _refs(pb, Z, N, Y, M, g, imu)
    vb = _vb(r["V"], batch)
    t = _tols(pb, r, N, M, g, imu, R.kernel_exp(vb))
    kw = dict(mu=mu, vbound=vb)
    print(f"\n(m, n, batch) = ({m}, {n}, {batch}), {kind}, c = {pb.c:.6g}")
    out = {}
    for path in ("i8", "f64", "f64_fused"):
        tp = "i8" if path == "i8" else "f64"
        out["A", path] = L.linop_host("A", path, pb.A, Z=Z, N=N, Y=Y, M=M, **kw)
        _check(R.err_against(out["A", path], *r["AV"], add=r["S"], sign=-1), t["A", tp], f"A {path}")
        out["AH", path] = L.linop_host("AH", path, pb.A, Z=Z, N=N, g=g, **kw)
        if path == "i8":
            _check(R.err_against(out["AH", path], *r["W"]), t["W", "i8"], "AH i8 (W)")
        else:
            _check(R.err_against(out["AH", path], *r["W"], add=r["V"]), t["X", "f64"], f"AH {path}")
    # setup: K against c^2 K_int (a GEMM of A with conj(A)), then K Y on both paths
    K, _, c = L.linop_host("setup", "i8", pb.A)
    assert c[0] == pb.c and c[1] == pb.c2
    Kid = pb.c2 * pb.Kint
    a1 = np.abs(pb.A.real) + np.abs(pb.A.imag)
    ktol = 2 * (n + 4) * R.U * (a1 @ a1.T) + R.U * np.abs(Kid.real) + R.U * np.abs(Kid.imag)
    dK = np.maximum(np.abs(K.real - Kid.real), np.abs(K.imag - Kid.imag))
    assert (dK <= ktol).all(), float((dK / ktol).max())
    assert np.array_equal(np.rint(K.real / pb.c2) + 1j * np.rint(K.imag / pb.c2), pb.Kint)
    out["K", "i8"] = L.linop_host("K", "i8", pb.A, g=g, **kw)
    _check(R.err_against(out["K", "i8"], *r["KY"]), t["K", "i8"], "K i8")
    out["K", "f64"] = L.linop_host("K", "f64", pb.A, g=g, **kw)
    kyf = R.exact_cmatvec(K, g)
    t["K", "f64"] = R.gemm_tol(K, g, C=out["K", "f64"])
    _check(R.err_against(out["K", "f64"], *kyf), t["K", "f64"], "K f64")
    # recipe 6: int8 against f64 (same exact reference for A and A^H; for K the f64 operator is the setup's K,
    # which differs from c^2 K_int by at most dK + u |c^2 K_int| per component)
    g1 = np.abs(g.real) + np.abs(g.imag)
    kx = np.repeat(g1 @ (2 * dK + 2 * R.U * (np.abs(Kid.real) + np.abs(Kid.imag))).T, 2, axis=1)
    for fp in ("f64", "f64_fused"):
        d = np.abs((out["A", "i8"] - out["A", fp]).view(np.float64))
        _check(d, t["A", "i8"] + t["A", "f64"], f"A i8 vs {fp}")
        xi8 = R.err_against(out["AH", fp], out["AH", "i8"].view(np.float64), np.zeros((batch, 2 * n)), add=r["V"])
        _check(xi8, t["W", "i8"] + t["X", "f64"], f"AH i8 vs {fp}")
    d = np.abs((out["K", "i8"] - out["K", "f64"]).view(np.float64))
    _check(d, t["K", "i8"] + t["K", "f64"] + kx, "K i8 vs f64")
    if m * n * batch <= PRIVATE_MAX:   # private codebooks (GEMV kernels): two different codes
        pb2 = Problem(m, n, "pmj" if kind != "pmj" else "synth", seed=1)
        r2 = _refs(pb2, Z, N, Y, M, g, imu)
        Ap = np.stack([(pb, pb2)[b % 2].A for b in range(batch)])
        odd = (np.arange(batch) % 2 == 1)[:, None]
        sel = lambda a, b: np.where(odd, b, a)   # noqa: E731
        o = L.linop_host("A", "f64", Ap, Z=Z, N=N, Y=Y, M=M, **kw)
        tA2 = (R.gemm_tol(pb2.A, r2["V"], E=r2["S"], C=r2["T"]) + R.pre_rounding(pb2.A, N, imu)
               + R.own_rounding(M, imu))
        _check(R.err_against(o, sel(r["AV"][0], r2["AV"][0]), sel(r["AV"][1], r2["AV"][1]), add=r["S"], sign=-1),
               sel(t["A", "f64"], tA2), "A private")
        o = L.linop_host("AH", "f64", Ap, Z=Z, N=N, g=g, **kw)
        tX2 = R.gemm_tol(pb2.A, g, E=r2["V"], C=r2["X"], herm=True) + R.own_rounding(N, imu)
        _check(R.err_against(o, sel(r["W"][0], r2["W"][0]), sel(r["W"][1], r2["W"][1]), add=r["V"]),
               sel(t["X", "f64"], tX2), "AH private")
        Kp, _, _ = L.linop_host("setup", "f64", Ap)
        o = L.linop_host("K", "f64", Ap, g=g, **kw)
        k0, k1 = R.exact_cmatvec(Kp[0], g), R.exact_cmatvec(Kp[min(1, batch - 1)], g)
        _check(R.err_against(o, sel(k0[0], k1[0]), sel(k0[1], k1[1])),
               sel(R.gemm_tol(Kp[0], g, C=o), R.gemm_tol(Kp[min(1, batch - 1)], g, C=o)), "K private")


# ------------------------------------------------------------------------------------------ recipe 3
EDGE_SHAPES = [(15, 33, 37, "synth"), (257, 64, 17, "pmj"), (300, 100, 17, "off")]


@pytest.mark.parametrize("m,n,batch,kind", EDGE_SHAPES, ids=[f"m{m}-n{n}-b{b}-{k}" for m, n, b, k in EDGE_SHAPES])
def test_exponent_edges_of_the_digit_planes(gpu, m, n, batch, kind):
    """vbound = max|v| an exact power of two, max|v| one ulp below a power of two, one component 2^40 times the
    rest: inside the tolerance at the kernel's exponent.  vbound = 2^10 max|v|: inside the tolerance at that
    exponent, with an error RMS of at most 1.25 times the uniform-rounding value c sqrt(N_nz / 12) 2^(e - 54).
    Zero vectors: T = S bit for bit, W = 0, K Y = 0."""
    L = _lin()
    rng = np.random.default_rng([3, m, n, batch])
    pb = Problem(m, n, kind)
    mu = np.ones(batch)
    Z, g = R.edge_vectors(rng, batch, n), R.edge_vectors(rng, batch, m)
    Y = R.rand_vectors(rng, batch, m, 0.0)
    AV = R.exact_matvec(pb.EA, Z.view(np.float64), pb.c)
    T = (Y.view(np.float64) - AV[0]).view(np.complex128)
    vb = R.maxabs_rows(Z)
    assert (np.frexp(vb[0::4])[0] == 0.5).all() and (np.frexp(np.nextafter(vb[1::4], np.inf))[0] == 0.5).all()
    print(f"\n(m, n, batch) = ({m}, {n}, {batch}), {kind}")
    out = L.linop_host("A", "i8", pb.A, Z=Z, Y=Y, mu=mu, vbound=vb)
    _check(R.err_against(out, *AV, add=Y, sign=-1), R.i8_tol(pb.EA, pb.c, R.kernel_exp(vb), AV[0], S=Y, T=T), "A edges")
    eg = R.kernel_exp(R.maxabs_rows(g))
    W = R.exact_matvec(pb.EH, g.view(np.float64), pb.c)
    _check(R.err_against(L.linop_host("AH", "i8", pb.A, g=g, mu=mu), *W), R.i8_tol(pb.EH, pb.c, eg, W[0]), "AH edges")
    KY = R.exact_matvec(pb.EK, g.view(np.float64), pb.c2)
    _check(R.err_against(L.linop_host("K", "i8", pb.A, g=g, mu=mu), *KY), R.i8_tol(pb.EK, pb.c2, eg, KY[0]), "K edges")
    # loose bound: vbound = 2^10 max|v|, Y = 0 so that T = -(A V) carries the product's error alone
    Zl = R.rand_vectors(rng, batch, n, 0.0)
    vbl = 1024.0 * R.maxabs_rows(Zl)
    el = R.kernel_exp(vbl)
    AVl = R.exact_matvec(pb.EA, Zl.view(np.float64), pb.c)
    out = L.linop_host("A", "i8", pb.A, Z=Zl, Y=np.zeros((batch, m)), mu=mu, vbound=vbl)
    err = R.err_against(out, *AVl, sign=-1)
    _check(err, R.i8_tol(pb.EA, pb.c, el, AVl[0], T=out), "A loose bound")
    live = np.abs(pb.EA).sum(axis=1) > 0
    assert err[:, live].size >= 1000
    ratio = float(np.sqrt(np.mean((err[:, live] / R.uniform_rms(pb.EA, pb.c, el)[:, live]) ** 2)))
    print(f"  A loose bound: error RMS / uniform-rounding value {ratio:.3f} over {err[:, live].size} outputs")
    assert ratio <= 1.25
    # zero vectors
    zn, zm = np.zeros((batch, n), np.complex128), np.zeros((batch, m), np.complex128)
    Mv = R.rand_vectors(rng, batch, m, 0.0)
    mu2, imu2 = _mu_imu(rng, batch)
    _same(L.linop_host("A", "i8", pb.A, Z=zn, Y=Y, M=Mv, mu=mu2, vbound=0.0), R.fma_ref(Mv, imu2, Y), "A v = 0: T = S")
    assert not L.linop_host("AH", "i8", pb.A, g=zm, mu=mu).view(np.float64).any()
    assert not L.linop_host("K", "i8", pb.A, g=zm, mu=mu).view(np.float64).any()


# ------------------------------------------------------------------------------------------ recipe 4
FLAG_SHAPES = [(257, 64, 17, "synth"), (300, 100, 17, "pmj")]


@pytest.mark.parametrize("m,n,batch,kind", FLAG_SHAPES, ids=[f"m{m}-n{n}-b{b}-{k}" for m, n, b, k in FLAG_SHAPES])
def test_isolation_and_flags(gpu, m, n, batch, kind):
    """Batch 17: vector 16 sits alone in its work-group, vector 3 among fifteen neighbours.  A non-finite bound
    or operand turns that vector's outputs to NaN and changes no other vector by a bit; done keeps the sentinel;
    nzero never reads N; avok takes A V = AX."""
    L = _lin()
    rng = np.random.default_rng([4, m, n, batch])
    pb = Problem(m, n, kind)
    mu, imu = _mu_imu(rng, batch)
    Z, N = R.rand_vectors(rng, batch, n), R.rand_vectors(rng, batch, n)
    Y, M, g = R.rand_vectors(rng, batch, m), R.rand_vectors(rng, batch, m), R.rand_vectors(rng, batch, m)
    V = R.fma_ref(N, imu, Z)
    vb = _vb(V, batch)
    base = {"A": L.linop_host("A", "i8", pb.A, Z=Z, N=N, Y=Y, M=M, mu=mu, vbound=vb),
            "AH": L.linop_host("AH", "i8", pb.A, g=g, mu=mu), "K": L.linop_host("K", "i8", pb.A, g=g, mu=mu)}
    others = lambda j: np.arange(batch) != j   # noqa: E731
    for j in (3, 16):
        for bad in (np.inf, np.nan):
            v2 = vb.copy()
            v2[j] = bad
            o = L.linop_host("A", "i8", pb.A, Z=Z, N=N, Y=Y, M=M, mu=mu, vbound=v2)
            assert np.isnan(o[j].view(np.float64)).all(), ("A vbound", j, bad)
            _same(o[others(j)], base["A"][others(j)], f"A vbound[{j}] = {bad}")
            for op in ("AH", "K"):
                g2 = g.copy()
                g2[j, (7 * j) % m] = complex(1.0, bad) if j == 3 else complex(bad, 1.0)
                o = L.linop_host(op, "i8", pb.A, g=g2, mu=mu)
                assert np.isnan(o[j].view(np.float64)).all(), (op, j, bad)
                _same(o[others(j)], base[op][others(j)], f"{op} operand[{j}] = {bad}")
    # done: the row keeps the sentinel, the others do not change
    done = np.zeros(batch, np.int32)
    done[[3, 16]] = 1
    sent = np.full((2, 1), L.SENTINEL * (1 + 1j))
    runs = [("A", "i8", dict(Z=Z, N=N, Y=Y, M=M, vbound=vb)), ("AH", "i8", dict(g=g)), ("K", "i8", dict(g=g)),
            ("A", "f64_fused", dict(Z=Z, N=N, Y=Y, M=M)), ("AH", "f64_fused", dict(Z=Z, N=N, g=g))]
    for op, path, kw in runs:
        o = L.linop_host(op, path, pb.A, mu=mu, done=done, **kw)
        ref = base[op] if path == "i8" else L.linop_host(op, path, pb.A, mu=mu, **kw)
        _same(o[[3, 16]], np.broadcast_to(sent, (2, o.shape[1])).copy(), f"{op} {path} done rows")
        _same(o[done == 0], ref[done == 0], f"{op} {path} live rows beside done ones")
        assert not (ref.view(np.float64) == L.SENTINEL).any()
    # nzero: N is not read (NaN-filled), the result is that of N = 0
    nz = np.zeros(batch, np.int32)
    nz[[0, 3, 16]] = 1
    Nn = N.copy()
    Nn[nz == 1] = complex(np.nan, np.nan)
    N0 = N.copy()
    N0[nz == 1] = 0.0
    vb0 = _vb(R.fma_ref(N0, imu, Z), batch)
    for path in ("i8", "f64"):
        _same(L.linop_host("A", path, pb.A, Z=Z, N=Nn, Y=Y, M=M, mu=mu, vbound=vb0, nzero=nz),
              L.linop_host("A", path, pb.A, Z=Z, N=N0, Y=Y, M=M, mu=mu, vbound=vb0), f"A {path} nzero")
    _same(L.linop_host("AH", "f64", pb.A, Z=Z, N=Nn, g=g, mu=mu, nzero=nz),
          L.linop_host("AH", "f64", pb.A, Z=Z, N=N0, g=g, mu=mu), "AH f64 nzero")
    # avok: T = S - AX exactly, in the mixed block (vectors 2, 3 of the first sixteen) and for vector 16
    AX = R.rand_vectors(rng, batch, m)
    av = np.zeros(batch, np.int32)
    av[[2, 3, 16]] = 1
    o = L.linop_host("A", "i8", pb.A, Z=Z, N=N, Y=Y, M=M, mu=mu, vbound=vb, AX=AX, avok=av)
    S = R.fma_ref(M, imu, Y)
    _same(o[av == 1], (S - AX)[av == 1], "A avok rows: T = S - AX")
    _same(o[av == 0], base["A"][av == 0], "A rows beside avok ones")
    _same(L.linop_host("A", "i8", pb.A, Z=Z, N=N, Y=Y, M=M, mu=mu, vbound=vb, AX=AX), base["A"], "A with AX, no avok")


# ------------------------------------------------------------------------------------------ recipe 5
def test_position_invariance(gpu):
    """A vector's output does not depend on where it sits: alone in a batch of 1, or at positions 5, 16 and 36 of
    a batch of 37 -- on every path; with rcols = 20 as column 0 and as column 19 of different realisations."""
    L = _lin()
    m, n = 121, 100
    rng = np.random.default_rng([5, m, n])
    pb = Problem(m, n, "synth")
    pb2 = Problem(m, n, "pmj", seed=1)
    z, nn, y, mm, g = (R.rand_vectors(rng, 1, k) for k in (n, n, m, m, m))
    mu1 = np.array([1.7])
    vb1 = _vb(R.fma_ref(nn, 1.0 / mu1, z), 1)
    Z, N = R.rand_vectors(rng, 37, n), R.rand_vectors(rng, 37, n)
    Y, M, G = R.rand_vectors(rng, 37, m), R.rand_vectors(rng, 37, m), R.rand_vectors(rng, 37, m)
    mu, imu = _mu_imu(rng, 37)
    pos = [5, 16, 36]
    for X, x in ((Z, z), (N, nn), (Y, y), (M, mm), (G, g)):
        X[pos] = x[0]
    mu[pos] = mu1[0]
    vb = _vb(R.fma_ref(N, 1.0 / mu, Z), 37)
    Ap1, Ap = pb.A[None], np.stack([pb.A if b in pos else pb2.A for b in range(37)])
    cases = [("A", p, pb.A, pb.A, dict(Z=z, N=nn, Y=y, M=mm), dict(Z=Z, N=N, Y=Y, M=M)) for p in ("f64", "f64_fused", "i8")]
    cases += [("AH", p, pb.A, pb.A, dict(Z=z, N=nn, g=g), dict(Z=Z, N=N, g=G)) for p in ("f64", "f64_fused", "i8")]
    cases += [("K", p, pb.A, pb.A, dict(g=g), dict(g=G)) for p in ("f64", "i8")]
    cases += [("G", "f64", pb.A, pb.A, dict(g=g), dict(g=G))]
    cases += [("A", "f64", Ap1, Ap, dict(Z=z, N=nn, Y=y, M=mm), dict(Z=Z, N=N, Y=Y, M=M)),
              ("AH", "f64", Ap1, Ap, dict(Z=z, N=nn, g=g), dict(Z=Z, N=N, g=G)),
              ("K", "f64", Ap1, Ap, dict(g=g), dict(g=G)), ("G", "f64", Ap1, Ap, dict(g=g), dict(g=G))]
    for op, path, A1, A37, k1, k37 in cases:
        one = L.linop_host(op, path, A1, mu=mu1, vbound=vb1, **k1)
        many = L.linop_host(op, path, A37, mu=mu, vbound=vb, **k37)
        for p in pos:
            _same(many[p:p + 1], one, f"{op} {path} {'private' if A1.ndim == 3 else 'shared'} position {p}")
    # rcols = 20: the vector as column 0 of realisation 1 and column 19 of realisation 2 (3 realisations, 60 vectors)
    rc, nb = 20, 3
    Z, N = R.rand_vectors(rng, nb * rc, n), R.rand_vectors(rng, nb * rc, n)
    Y, M, G = R.rand_vectors(rng, nb * rc, m), R.rand_vectors(rng, nb * rc, m), R.rand_vectors(rng, nb * rc, m)
    pos = [20, 59]
    for X, x in ((Z, z), (N, nn), (Y, y), (M, mm), (G, g)):
        X[pos] = x[0]
    mu = np.array([0.9, mu1[0], mu1[0]])
    vb = _vb(R.fma_ref(N, R.per_vector(1.0 / mu, nb * rc, rc), Z), nb)
    vb[1:] = vb[1:].max()   # (one exponent for the two placements)
    for op, k1, k60 in (("A", dict(Z=z, N=nn, Y=y, M=mm), dict(Z=Z, N=N, Y=Y, M=M)),
                        ("AH", dict(Z=z, N=nn, g=g), dict(Z=Z, N=N, g=G)), ("K", dict(g=g), dict(g=G))):
        for path in ("i8", "f64"):
            one = L.linop_host(op, path, pb.A, mu=mu1, vbound=vb[1:2], rcols=1, **k1)
            many = L.linop_host(op, path, pb.A, mu=mu, vbound=vb, rcols=rc, **k60)
            if op == "AH" and path == "i8":   # rcols = 1 returns W, the r-column form X = V + W
                v1 = R.fma_ref(nn, 1.0 / mu1, z)
                one = (v1.view(np.float64) + one.view(np.float64)).view(np.complex128)
            _same(many[20:21], many[59:60], f"{op} {path} rcols = 20: column 0 against column 19")
            _same(many[20:21], one, f"{op} {path} rcols = 20 against rcols = 1")


# ------------------------------------------------------------------------------------------ r-column stages
def test_rcols_20_per_realisation_state(gpu):
    """rcols = 20 with 3 realisations (60 vectors, not a multiple of 16), each with its own mu and vbound; one
    realisation done, one with nzero and a NaN-filled N: integer data bit-exact, full-mantissa data within the
    derived tolerance on the int8 r-column launches and the f64 GEMM."""
    L = _lin()
    m, n, nb, rc = 15, 33, 3, 20
    nv = nb * rc
    rng = np.random.default_rng([6, m, n])
    # integer data, c = 1
    pb = Problem(m, n, "pmj1", unit=True)
    mu = np.array([1.0, 2.0, 4.0])
    imu = R.per_vector(1.0 / mu, nv, rc)
    muv = R.per_vector(mu, nv, rc)
    Z, Y, g = R.int_vectors(rng, nv, n, 19), R.int_vectors(rng, nv, m, 19), R.int_vectors(rng, nv, m, 20)
    N, M = R.int_vectors(rng, nv, n, 19) * muv[:, None], R.int_vectors(rng, nv, m, 19) * muv[:, None]
    V, S = Z - N * imu[:, None], Y - M * imu[:, None]

    def iprod(E, X):
        return (X.view(np.float64).astype(np.int64) @ E.astype(np.int64).T).astype(np.float64).view(np.complex128)
    kw = dict(mu=mu, vbound=_vb(V, nb), rcols=rc)
    for path in ("i8", "f64"):
        _same(L.linop_host("A", path, pb.A, Z=Z, N=N, Y=Y, M=M, **kw), S - iprod(pb.EA, V), f"A {path} rcols")
        _same(L.linop_host("AH", path, pb.A, Z=Z, N=N, g=g, **kw), V + iprod(pb.EH, g), f"AH {path} rcols")
        _same(L.linop_host("K", path, pb.A, g=g, **kw), iprod(pb.EK, g), f"K {path} rcols")
    # full-mantissa data, per-realisation mu and vbound, flags
    pb = Problem(m, n, "synth")
    mu = np.array([0.6, 1.9, 3.3])
    imu = R.per_vector(1.0 / mu, nv, rc)
    Z, N = R.rand_vectors(rng, nv, n), R.rand_vectors(rng, nv, n)
    Y, M, g = R.rand_vectors(rng, nv, m), R.rand_vectors(rng, nv, m), R.rand_vectors(rng, nv, m)
    nz, done = np.array([0, 0, 1], np.int32), np.array([0, 1, 0], np.int32)
    N0 = N.copy()
    N0[2 * rc:] = 0.0
    Nn = N.copy()
    Nn[2 * rc:] = complex(np.nan, np.nan)
    r = _refs(pb, Z, N0, Y, M, g, imu)
    vb = _vb(r["V"], nb) * np.array([1.0, 1.0, 3.0])   # (a loose bound on the last realisation)
    t = _tols(pb, r, N0, M, g, imu, R.per_vector(R.kernel_exp(vb), nv, rc).astype(np.int64))
    live = np.repeat(done == 0, rc)
    sent = L.SENTINEL * (1 + 1j)
    kw = dict(mu=mu, vbound=vb, rcols=rc, nzero=nz, done=done)
    print()
    for path in ("i8", "f64"):
        o = L.linop_host("A", path, pb.A, Z=Z, N=Nn, Y=Y, M=M, **kw)
        _check(R.err_against(o, *r["AV"], add=r["S"], sign=-1)[live], t["A", path][live], f"A {path} rcols = 20")
        o2 = L.linop_host("AH", path, pb.A, Z=Z, N=Nn, g=g, **kw)
        _check(R.err_against(o2, *r["W"], add=r["V"])[live], t["X", path][live], f"AH {path} rcols = 20")
        if path == "i8":
            assert (o[~live] == sent).all() and (o2[~live] == sent).all()
            o3 = L.linop_host("K", "i8", pb.A, g=g, **kw)
            _check(R.err_against(o3, *r["KY"])[live], t["K", "i8"][live], "K i8 rcols = 20")
            assert (o3[~live] == sent).all()


# ------------------------------------------------------------------------------------------ G
def _ref_probe_rows(rows):
    p = np.load(ROOT / "tests" / "golden" / "ref_codebooks_16x16_packed.npz")["random"][:rows]
    k = np.stack([(p >> (2 * i)) & 3 for i in range(4)], axis=-1).reshape(rows, -1).astype(np.int64)
    return (np.array([1, 0, -1, 0])[k] + 1j * np.array([0, 1, 0, -1])[k]) / np.sqrt(k.shape[1])


@pytest.mark.parametrize("name", ["synth-121x65", "pmj-300x100", "probe-400x256"])
def test_g_newton_schulz(gpu, name):
    """g = G T with the shared Newton-Schulz G: the apply within the GEMM tolerance of the exact product with the
    G the setup left, and G T within gamma_m kappa_inf(I + K) ||g*||_inf of the longdouble solution g* -- on
    vectors that attain ||B^-1 T|| = ||B^-1|| ||T|| and on random ones.  probe-400x256: the first 400 rows of the
    reference's probing codebook (m > n, K rank-deficient, the structure on which a first-order iteration diverged)."""
    L = _lin()
    A = {"synth-121x65": lambda: R.codebook("synth", 121, 65), "pmj-300x100": lambda: R.codebook("pmj", 300, 100),
         "probe-400x256": lambda: _ref_probe_rows(400)}[name]()
    m = A.shape[0]
    rng = np.random.default_rng([7, m])
    K, G, _ = L.linop_host("setup", "f64", A)
    _same(G, G.conj().T, "G Hermitian")
    _, kappa, Binv = R.g_reference(K, np.zeros((1, m)))
    T = np.concatenate([R.norm_attaining(Binv, 4), R.rand_vectors(rng, 13, m, 0.0)])
    gs, kappa, _ = R.g_reference(K, T)
    out = L.linop_host("G", "f64", A, g=T)
    ex = R.exact_cmatvec(G, T)
    print(f"\n{name}: kappa_inf(I + K) = {kappa:.4g}, gamma_m = {R.gamma_m(m):.3g}")
    _check(R.err_against(out, *ex), R.gemm_tol(G, T, C=out), "G apply against the exact G T")
    gG = (ex[0].astype(np.longdouble) + ex[1].astype(np.longdouble)).view(np.clongdouble)
    err = np.max(np.abs(gG - gs), axis=1).astype(np.float64)[:, None]
    bound = (R.gamma_m(m) * kappa * np.max(np.abs(gs), axis=1).astype(np.float64))[:, None]
    _check(err[:4], bound[:4], "G T against g*, norm-attaining T")
    _check(err[4:], bound[4:], "G T against g*, random T")


def test_g_gauss_jordan_private(gpu):
    """Private codebooks: G_b by Gauss-Jordan, two different codes; the GEMV apply against the exact product with
    the G_b read back, and G_b T against the longdouble solution."""
    L = _lin()
    m, n, batch = 121, 65, 5
    rng = np.random.default_rng([8, m])
    codes = [R.codebook("synth", m, n), R.codebook("pmj", m, n, seed=1)]
    Ap = np.stack([codes[b % 2] for b in range(batch)])
    K, G, _ = L.linop_host("setup", "f64", Ap)
    T = R.rand_vectors(rng, batch, m, 0.0)
    out = L.linop_host("G", "f64", Ap, g=T)
    print()
    for b in range(batch):
        ex = R.exact_cmatvec(G[b], T[b:b + 1])
        _check(R.err_against(out[b:b + 1], *ex), R.gemm_tol(G[b], T[b:b + 1], C=out[b:b + 1]), f"G private apply [{b}]")
        gs, kappa, _ = R.g_reference(K[b], T[b:b + 1])
        gG = (ex[0].astype(np.longdouble) + ex[1].astype(np.longdouble)).view(np.clongdouble)
        err = np.max(np.abs(gG - gs), axis=1).astype(np.float64)[:, None]
        _check(err, (R.gamma_gj(m) * kappa * np.max(np.abs(gs), axis=1).astype(np.float64))[:, None],
               f"G_b T against g* [{b}]")


# ------------------------------------------------------------------------------------------ the entry itself
def test_int8_path_is_refused_not_replaced(gpu):
    """A codebook that is not a phase code: the int8 path returns ACE_ERR_UNSUPPORTED (no fall-back to f64)."""
    from ace_amd import _lib
    L = _lin()
    rng = np.random.default_rng(9)
    A = R.codebook("synth", 15, 33)
    A[3, 4] *= 0.5
    g = R.rand_vectors(rng, 4, 15)
    with pytest.raises(_lib.AceError) as ei:
        L.linop_host("K", "i8", A, g=g)
    assert ei.value.code == _lib.ACE_ERR_UNSUPPORTED
    assert L.linop_host("K", "f64", A, g=g).shape == (4, 15)
    with pytest.raises(_lib.AceError):
        L.linop_host("G", "i8", R.codebook("synth", 15, 33), g=g)


# ------------------------------------------------------------------------------------------ raw GEMM
def _gemm_ref(mode, conj_l, Lm, V, E):
    acc = np.einsum("zik,zbk->zbi", Lm.conj() if conj_l else Lm, V)
    return acc if mode == 0 else (E - acc if mode == 1 else E + acc)


def _gemm_run(mode, conj_l, M, K, nb, nz, rng, pad=(0, 0, 0), zpad=(0, 0, 0), klim=None):
    """One launch on integer data in padded arrays: NaN in the padding of L and V (a read outside the operand
    shows), a sentinel in C's (a write outside shows).  Returns (got, expected) over the whole C array."""
    L = _lin()
    ldl, ldv, ldc = K + pad[0], K + pad[1], M + pad[2]
    sL, sV, sC = M * ldl + zpad[0], nb * ldv + zpad[1], nb * ldc + zpad[2]
    Lm = (rng.integers(-1000, 1001, (nz, M, K)) + 1j * rng.integers(-1000, 1001, (nz, M, K))).astype(np.complex128)
    V = (rng.integers(-2 ** 20, 2 ** 20, (nz, nb, K)) + 1j * rng.integers(-2 ** 20, 2 ** 20, (nz, nb, K))).astype(np.complex128)
    E = (rng.integers(-2 ** 30, 2 ** 30, (nz, nb, M)) + 1j * rng.integers(-2 ** 30, 2 ** 30, (nz, nb, M))).astype(np.complex128)
    if klim is not None:
        for z in range(nz):
            Lm[z, :, int(klim[z]):] = 0.0
            V[z, :, int(klim[z]):] = 0.0
    nanc, sent = complex(np.nan, np.nan), complex(-3.5e55, 4.5e44)

    def pack(X, rows, cols, ld, stride, fill):
        buf = np.full(nz * stride, fill, np.complex128)
        for z in range(nz):
            buf[z * stride:z * stride + rows * ld].reshape(rows, ld)[:, :cols] = X[z]
        return buf
    Lb, Vb = pack(Lm, M, K, ldl, sL, nanc), pack(V, nb, K, ldv, sV, nanc)
    Eb = pack(E, nb, M, ldc, sC, nanc)
    Cb = np.full(nz * sC, sent, np.complex128)
    got = L.zgemm_host(mode, conj_l, M, K, nb, Lb, Vb, Cb, None if mode == 0 else Eb, ldl=ldl, ldv=ldv, ldc=ldc,
                       strideL=sL, strideV=sV, strideC=sC, nz=nz, klim=klim, klim_stride=1 if klim is not None else 0)
    return got, pack(_gemm_ref(mode, conj_l, Lm, V, E), nb, M, ldc, sC, sent)


GEMM_SHAPES = [(1, 1, 1), (31, 15, 63), (32, 16, 64), (33, 17, 65), (64, 100, 1), (65, 15, 65), (1, 100, 64),
               (31, 17, 1), (33, 1, 63), (64, 16, 65), (65, 100, 63), (32, 15, 64)]


@pytest.mark.parametrize("M,K,nb", GEMM_SHAPES, ids=[f"M{a}-K{b}-nb{c}" for a, b, c in GEMM_SHAPES])
def test_zgemm_modes_and_tails(gpu, M, K, nb):
    """Every mode and conjugation at tile tails in M, K and nb, with non-trivial leading dimensions: integer data,
    bit-exact over the whole C array (the padding keeps its sentinel)."""
    rng = np.random.default_rng([10, M, K, nb])
    for mode in (0, 1, 2):
        for conj_l in (False, True):
            got, exp = _gemm_run(mode, conj_l, M, K, nb, 1, rng, pad=(3, 1, 2))
            _same(got[None], exp[None], f"zgemm mode {mode} conj {conj_l}")


def test_zgemm_big_tile_strides_and_klim(gpu):
    """M = 65, nb = 65, nz = 64 is 256 blocks of the 64 x 64 tile (the Big configuration); a z-batched launch
    with padded leading dimensions and z strides; a launch with a per-slice summation limit (operands zero beyond)."""
    rng = np.random.default_rng(11)
    for mode, conj_l in ((0, True), (1, False), (2, True)):
        got, exp = _gemm_run(mode, conj_l, 65, 17, 65, 64, rng, pad=(1, 2, 3), zpad=(5, 7, 11))
        _same(got[None], exp[None], f"zgemm Big tile mode {mode}")
    got, exp = _gemm_run(2, False, 33, 100, 17, 5, rng, pad=(4, 0, 1), zpad=(9, 3, 0))
    _same(got[None], exp[None], "zgemm z-batched, Small tile")
    for M, nb, nz in ((33, 17, 6), (65, 65, 64)):
        klim = np.array(([100.0, 0.0, 1.0, 16.0, 17.0, 99.0] * 11)[:nz])
        got, exp = _gemm_run(0, True, M, 100, nb, nz, rng, pad=(0, 2, 0), zpad=(1, 0, 2), klim=klim)
        _same(got[None], exp[None], f"zgemm klim, nz = {nz}")


def test_zgemm_full_mantissa_within_tolerance(gpu):
    """Full-mantissa operands: every output within the 3M tolerance of the exact product."""
    L = _lin()
    rng = np.random.default_rng(12)
    print()
    for M, K, nb in ((33, 100, 17), (65, 17, 65)):
        Lm, V, E = R.rand_vectors(rng, M, K, 2.0), R.rand_vectors(rng, nb, K), R.rand_vectors(rng, nb, M)
        for mode, conj_l in ((0, False), (1, True), (2, False)):
            C = L.zgemm_host(mode, conj_l, M, K, nb, Lm, V, np.zeros((nb, M)), None if mode == 0 else E,
                             ldl=K, ldv=K, ldc=M).reshape(nb, M)
            ex = R.exact_cmatvec(Lm.conj() if conj_l else Lm, V)
            add, sign = (None, 1) if mode == 0 else (E, -1 if mode == 1 else 1)
            _check(R.err_against(C, *ex, add=add, sign=sign), R.gemm_tol(Lm, V, E=add, C=C),
                   f"zgemm M {M} K {K} nb {nb} mode {mode} conj {conj_l}")
