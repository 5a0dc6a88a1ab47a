"""The Z-step kernels on their own against the extended-precision reference of tests/zprox_ref.py:

    Z' = ArgMinZ(X + N/mu)      N' = N + mu (X - Z')      iteration control      (inferLowRankV4_multi.m:423-485, :344-381)

through the test entry ace_zprox_host (ace_amd.zprox), which fills the Z-step argument block and one control block
per realisation as a solve does and calls the solve's launcher: the one-wave kernel at r = 1 (Jacobi cold and warm,
the tridiagonal top-K path, the rank-one Lanczos path, the Ky Fan certificate, the wmode / ping-pong form, the lean
kernel, the A2nuclear soft threshold), the four-wave kernel at r > 1 (its tx, rx <= 16 form and its 32 x 32 form,
zcert, tkeig).

Assertions (numbered as in DESIGN section 6): 1 Z' and N' inside the derived tolerance TOL_MULT u kappa on every
path; 2 no rescaling => Z' = E bit for bit (wmode: nzero, avok, N' untouched); 3 certificate soundness at
f (1 +- delta); 4 vbound >= max |Z' - N'/mu'| and NaN for non-finite input; 5 iteration control; 6 degenerate
spectra; 7 untouched memory.  Every comparison states its ratio err / tol (printed; the worst per path is in DESIGN, and is printed again when
the module finishes).
The inputs, their firing patterns, decision margins and boundary gaps are shown on the reference alone by
tests/test_zprox_ref.py.
"""
import math

import numpy as np
import pytest

import zprox_ref as R

pytestmark = pytest.mark.gpu

ACE_ST_CONVERGED = 1
WORST = {}   # path -> worst err / tol seen (printed by the last test)
SLACK = {}   # path -> worst vbound / true max


class _Entry:
    """ace_amd.zprox with one rule added: a HIP error ends the session (nothing more is launched on a device
    that has reported a fault)."""

    def __init__(self):
        from ace_amd import zprox
        self._z = zprox
        self.SENTINEL = zprox.SENTINEL

    def zprox_host(self, *a, **kw):
        from ace_amd import AceError
        try:
            return self._z.zprox_host(*a, **kw)
        except AceError as e:
            if e.code == -3:
                pytest.exit(f"HIP error in ace_zprox_host: {e}", returncode=3)
            raise


def _zp():
    return _Entry()


def _bits_equal(a, b):
    af, bf = np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64)
    return af.shape == bf.shape and bool(np.all((af.view(np.uint64) == bf.view(np.uint64)) | ((af == 0) & (bf == 0))))


def _sentinel(x, s):
    return bool(np.all(np.ascontiguousarray(x).view(np.float64) == s))


def _note(path, ratio):
    WORST[path] = max(WORST.get(path, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    """After the module's tests (whichever were selected): the worst err / tol per path and the vbound slack over
    the comparisons that ran (pytest -s shows them; DESIGN section 6 records a full run).  Every figure was asserted
    where it was measured; nothing is asserted here."""
    yield
    for k in sorted(WORST):
        print(f"  worst err/tol {k}: {WORST[k]:.3g}")
    for k in sorted(SLACK):
        print(f"  vbound slack {k}: {SLACK[k]:.4g}")


def _check_z(Zb, ref, tx, label, path):
    """One realisation's Z' ([r][n]) against its reference: bit-equal to E when nothing fires, else inside tol."""
    Zm = R.to_E(Zb, tx)
    assert np.all(np.isfinite(Zm.view(np.float64))), label
    if not ref.any_fired:
        assert _bits_equal(Zm, ref.E), f"{label}: no rescaling fires but Z' != E"
        return 0.0
    err = ref.err(Zm)
    ratio = err / ref.tol
    print(f"  {label} [{path}]: err/tol {ratio:.3g} (kappa {ref.kappa:.3g})")
    _note(path, ratio)
    assert err <= ref.tol, f"{label} [{path}]: err {err:.3e} > tol {ref.tol:.3e}"
    assert not _bits_equal(Zm, ref.E), f"{label}: a rescaling fires but Z' = E"
    return ratio


def _check_vbound(res, b, Znew, Nnew, path, label):
    """vbound >= max |Re, Im of Z' - N'/mu'| with the updated mu (extended precision, no rounding in favour)."""
    ld = np.longdouble
    mu = ld(res.mu[b])
    z = np.ascontiguousarray(Znew).view(np.float64).astype(ld)
    nn = np.ascontiguousarray(Nnew).view(np.float64).astype(ld)
    true = float(np.max(np.abs(z - nn / mu))) if z.size else 0.0
    vb = float(res.vbound[b])
    assert vb >= true, f"{label} [{path}]: vbound {vb!r} < max|Z' - N'/mu'| {true!r}"
    if true > 0:
        SLACK[path] = max(SLACK.get(path, 0.0), vb / true)


def _eig_q(E, perturb=0.0, seed=0):
    """Eigenvectors of (a perturbation of) E E^H, columns in descending eigenvalue order: a warm start."""
    rng = np.random.default_rng(seed)
    Ep = E + perturb * np.linalg.norm(E) / math.sqrt(E.size) * (rng.standard_normal(E.shape) + 1j * rng.standard_normal(E.shape))
    w, Q = np.linalg.eigh(Ep @ Ep.conj().T)
    return np.ascontiguousarray(Q[:, ::-1])


def _kw(case):
    """Entry arguments that select the case's profile: the entry derives it from m; rank-one by the flags."""
    kw = dict(r=case.r, m=case.m())
    if case.kind == "r1":
        kw["rank_one"] = 1
    return kw


ONEWAVE = R.CASES_1W + R.CASES_R1
IDS_1W = [c.name for c in ONEWAVE]
PATHS_1W = {"jacobi": dict(tkeig=0, r1lz=False), "topk": dict(tkeig=1000, r1lz=False), "r1lz": dict(tkeig=0, r1lz=True)}


def _paths_for(case):
    return ("jacobi", "r1lz") if case.kind == "r1" else ("jacobi", "topk")


# ------------------------------------------------------------------------------------------------ 1, 2, 4: init form
@pytest.mark.parametrize("case", ONEWAVE, ids=IDS_1W)
def test_init_form_one_wave(gpu, case):
    """Init Z-step (mu = 1, N = 0): every realisation runs the eigensolver (no certificate in the init form)."""
    refs = R.case_refs(case)
    X = case.X()
    for path in _paths_for(case):
        res = _zp().zprox_host(X, case.tx, case.rx, init=True, **_kw(case), **PATHS_1W[path])
        for b, ref in enumerate(refs):
            _check_z(res.Z[b], ref, case.tx, f"{case.name}[{b}] init", "1w-" + path)
            _check_vbound(res, b, res.Z[b], np.zeros_like(res.Z[b]), "1w-" + path, case.name)
        assert not res.N.any() and np.all(res.status == 0)
        if path == "topk":
            maxr = max(case.profile()[0])
            want = case.batch if (maxr <= 16 and case.tx >= 2) else 0
            assert res.tkcnt.tolist() == [want, 0], (case.name, res.tkcnt)   # used, and no fallback to Jacobi
        else:
            assert res.tkcnt.tolist() == [0, 0]


# ------------------------------------------------------------------------- 1, 2, 4: iteration form, in place, N != 0
def _iter_inputs(case, seed, with_n=True):
    """X of the case, a previous Z near it, N of size ~ mu |X| / 4 and one mu per realisation."""
    rng = np.random.default_rng(seed)
    X = case.X()
    Z0 = X + 0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    mu = np.array([0.37, 1.9, 0.011, 5.5][: case.batch] if case.batch <= 4 else rng.uniform(0.01, 3.0, case.batch))
    N = 0.25 * mu[:, None, None] * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    if not with_n:
        N = np.zeros_like(X)
    return X, Z0, N, mu


@pytest.fixture(scope="module")
def refs_with_n():
    """References of E = X + N/mu (exact) for the cases run with N != 0: computed once."""
    out = {}
    for case in (R.CASES_1W[2], R.CASES_1W[3], R.CASES_R1[0], R.CASES_4W[0], R.CASES_4W[1]):
        X, Z0, N, mu = _iter_inputs(case, 77)
        rl, fl = case.profile()
        refs = []
        for b in range(case.batch):
            E, dE = R.exact_E(R.to_E(X[b], case.tx), R.to_E(N[b], case.tx), mu[b])
            refs.append(R.argmin_z_ref(E, rl, fl, dE))
            assert refs[-1].margin >= 1e-6 and (not refs[-1].any_fired or refs[-1].gap >= 1e-3), (case.name, b)
        out[case.name] = (X, Z0, N, mu, refs)
    return out


def _check_n(res, b, case, X, N, mu, ref, path, label):
    """N' = N + mu (X - Z') within mu tol_Z ||E|| plus the roundings of the update."""
    Xe, Ne = R.to_E(X[b], case.tx), R.to_E(N[b], case.tx)
    want = R.n_update_ref(Ne, mu[b], Xe, ref)
    got = R.to_E(res.N[b], case.tx)
    err = float(np.linalg.norm((got.astype(np.clongdouble) - want).astype(np.complex128)))
    tol = R.n_tol(got, mu[b], Xe, R.to_E(res.Z[b], case.tx), ref)
    _note(path + "-N", err / tol)
    assert err <= tol, f"{label} [{path}]: N' err {err:.3e} > tol {tol:.3e}"


@pytest.mark.parametrize("name", ["8x8", "16x16", "16x16-r1"])
@pytest.mark.parametrize("mode", ["cold", "warm"])
def test_iteration_in_place_with_n(gpu, refs_with_n, name, mode):
    case = next(c for c in ONEWAVE if c.name == name)
    X, Z0, N, mu, refs = refs_with_n[name]
    Q = None
    if mode == "warm":
        Q = np.stack([_eig_q(r.E, 1e-3, b) for b, r in enumerate(refs)])
    for path in _paths_for(case):
        tag = f"1w-{path}-{mode}"
        res = _zp().zprox_host(X, case.tx, case.rx, Z=Z0, N=N, mu=mu, Q=Q, warm=mode == "warm", it=3, last_res=1e300,
                               **_kw(case), **PATHS_1W[path])
        for b, ref in enumerate(refs):
            label = f"{name}[{b}] it"
            if ref.any_fired:
                _check_z(res.Z[b], ref, case.tx, label, tag)
                _check_n(res, b, case, X, N, mu, ref, tag, label)
            else:
                # Z' = E = fma(N, fl(1/mu), X) as the kernel rounds it: one rounding of E and one of 1/mu
                Zm = R.to_E(res.Z[b], case.tx)
                assert np.all(np.abs(Zm - ref.Z_hi) <= 2 * R.U * (np.abs(ref.Z_hi) + np.abs(R.to_E(N[b], case.tx)) / mu[b])), label
                # N' = N + mu (X - E) is what those roundings leave: with E = (X + N i)(1 + d), i = (1 + e) / mu,
                # N' = -e N - mu d E and the three roundings of the update: <= u mu |X| + 4.5 u |N|
                lim = 4 * R.U * mu[b] * np.abs(X[b]).max() + 5 * R.U * np.abs(N[b]).max()
                assert np.abs(res.N[b].view(np.float64)).max() <= lim, (label, np.abs(res.N[b]).max(), lim)
            _check_vbound(res, b, res.Z[b], res.N[b], tag, label)
            assert res.mu[b] == mu[b] and res.iters[b] == 3      # last_res = 1e300: no mu update
            if mode == "warm" and ref.any_fired:
                q = res.Q[b]
                assert np.abs(q.conj().T @ q - np.eye(case.tx)).max() <= 1e-13, label   # the next warm start is unitary


# ------------------------------------------------------------------ 1, 2, 4: wmode, ping-pong outputs, N = 0 (nzero)
def _wmode_inputs(case):
    """Z0 = X rounded to f32 and W = X - Z0 (exact), so that the kernel's X = Z0 + W is the case's X bit for bit."""
    X = case.X()
    Z0 = X.astype(np.complex64).astype(np.complex128)
    W = X - Z0
    assert np.array_equal(Z0 + W, X)
    return X, Z0, W


@pytest.mark.parametrize("case", ONEWAVE, ids=IDS_1W)
def test_wmode_pingpong_warm(gpu, case):
    """Warm start = the eigenvectors of E E^H: realisations without a rescaling pass the Ky Fan certificate (Z' = E
    bit for bit, N' left alone, nzero = avok = 1), the others run the eigensolver on F = Q^H E."""
    zp = _zp()
    refs = R.case_refs(case)
    X, Z0, W = _wmode_inputs(case)
    Q = np.stack([_eig_q(r.E) for r in refs])
    junk = np.full_like(X, 3e300 + 3e300j)    # nzero = 1: the N buffer must not be read
    for path in _paths_for(case):
        tag = f"1w-{path}-wmode"
        res = zp.zprox_host(W, case.tx, case.rx, Z=Z0, N=junk, nzero=1, Q=Q, warm=True, wmode=True, pingpong=True, it=2,
                            mu=0.8, last_res=1e300, **_kw(case), **PATHS_1W[path])
        for b, ref in enumerate(refs):
            label = f"{case.name}[{b}] wmode"
            _check_z(res.Z[b], ref, case.tx, label, tag)
            if ref.any_fired:
                assert res.nzero[b] == 0 and res.avok[b] == 0 and res.kfok[b] == 0, label
                _check_n(res, b, case, X, np.zeros_like(X), np.full(case.batch, 0.8), ref, tag, label)
                _check_vbound(res, b, res.Z[b], res.N[b], tag, label)
            else:
                assert res.nzero[b] == 1 and res.avok[b] == 1, (label, res.nzero[b], res.avok[b])
                assert _sentinel(res.N[b], zp.SENTINEL), f"{label}: N' written although N' = 0 is implied"
                _check_vbound(res, b, res.Z[b], np.zeros_like(res.Z[b]), tag, label)
                if max(case.profile()[0]) <= 16:
                    assert res.kfok[b] == 1 and np.all(res.kf[b, : len(case.profile()[0])] > 0), label
                # the N' that is not stored: the reference's is at rounding level
                nref = R.n_update_ref(np.zeros_like(ref.E), 0.8, ref.E, ref)
                assert float(np.abs(nref).max()) <= 4 * R.U * 0.8 * np.abs(X[b]).max(), label
        assert np.all((res.status & ~ACE_ST_CONVERGED) == 0)


def test_wmode_cold_and_nonzero_n(gpu):
    """wmode without a warm start and with N != 0 on entry (nzero = 0): X = fl(fl(Z - N/mu) + W) as every producer
    of X rounds it; N' is stored, nzero = avok = 0 unless the certificate passes."""
    case = R.CASES_1W[2]   # 8x8
    rng = np.random.default_rng(9)
    rl, fl = case.profile()
    Xc = case.X()
    mu = np.array([0.6, 1.7, 0.2])
    N = 0.2 * mu[:, None, None] * (rng.standard_normal(Xc.shape) + 1j * rng.standard_normal(Xc.shape))
    Z0 = Xc + 0.03 * (rng.standard_normal(Xc.shape) + 1j * rng.standard_normal(Xc.shape))
    W = Xc - Z0
    X = np.stack([R.xw_ref(Z0[b], N[b], W[b], mu[b]) for b in range(3)])
    refs = []
    for b in range(3):
        E, dE = R.exact_E(R.to_E(X[b], 8), R.to_E(N[b], 8), mu[b])
        refs.append(R.argmin_z_ref(E, rl, fl, dE))
    res = _zp().zprox_host(W, 8, 8, Z=Z0, N=N, mu=mu, wmode=True, pingpong=True, it=5, last_res=1e300, **_kw(case))
    for b, ref in enumerate(refs):
        label = f"8x8[{b}] wmode cold N"
        if ref.any_fired:
            _check_z(res.Z[b], ref, 8, label, "1w-jacobi-wmode-N")
            _check_n(res, b, case, X, N, mu, ref, "1w-jacobi-wmode-N", label)
        else:
            assert np.all(np.abs(R.to_E(res.Z[b], 8) - ref.Z_hi)
                          <= 2 * R.U * (np.abs(ref.Z_hi) + np.abs(R.to_E(N[b], 8)) / mu[b])), label
        assert res.avok[b] == 0, label
        _check_vbound(res, b, res.Z[b], res.N[b] if res.nzero[b] == 0 else np.zeros_like(res.Z[b]), "1w-jacobi-wmode-N",
                      label)


# ------------------------------------------------------------------------------------------------ mixed rank_one flags
def test_mixed_rank_one_flags(gpu):
    """One batch, per-realisation profiles: flags (0, 1, 0) and (1, 0, 1) on the 16 x 16 inputs."""
    case = R.CASES_1W[3]
    X = case.X()
    full = R.case_refs(case)
    rl1, fl1 = R.profile_of(16, 16, "r1")
    one = [R.argmin_z_ref(R.to_E(X[b], 16), rl1, fl1) for b in range(3)]
    for flags in ((0, 1, 0), (1, 0, 1)):
        for path, kw in (("jacobi", dict()), ("r1lz+topk", dict(r1lz=True, tkeig=1000))):
            res = _zp().zprox_host(X, 16, 16, init=True, rank_one=np.array(flags, np.uint8), **kw)
            for b in range(3):
                _check_z(res.Z[b], one[b] if flags[b] else full[b], 16, f"16x16[{b}] flags {flags}", "1w-mixed-" + path)


# ------------------------------------------------------------------------------------------------ nuclear r = 1
def test_nuclear_soft_threshold(gpu):
    """A2nuclear at r = 1: Z = E max(0, ||E|| - 1/mu) / ||E||, including ||E|| <= 1/mu => Z = 0.  Tolerance per
    component: u |e| (8 + (16 + log2 n) g) with g = ||E|| / (||E|| - 1/mu) the cancellation of the subtraction:
    the norm is a sum of n squares (tree of depth log2 n plus 16 per-lane terms), one square root, one
    subtraction, one division, one product."""
    case = R.CASES_1W[4]   # 16x8
    X = case.X()
    nrm = np.array([np.linalg.norm(x) for x in X])
    mu = np.array([4.0 / nrm[0], 0.5 / nrm[1], 1.25 / nrm[2]])    # threshold at 1/4, 2 (Z = 0) and 4/5 of ||E||
    for init in (True, False):
        m_ = np.ones(3) if init else mu
        kw = dict(init=True) if init else dict(Z=X * 0.9, mu=mu, it=1, last_res=1e300)
        res = _zp().zprox_host(X, 16, 8, variant="A2nuclear", **kw)
        for b in range(3):
            imu = 1.0 / m_[b]
            f = max(0.0, nrm[b] - imu) / nrm[b]
            want = X[b] * f
            if f == 0.0:
                assert not res.Z[b].any(), b
                continue
            g = nrm[b] / (nrm[b] - imu)
            tol = R.U * np.abs(X[b]) * (8 + (16 + math.log2(case.n)) * g)
            d = np.abs(res.Z[b] - want)
            _note("1w-nuclear", float((d / tol).max()))
            assert np.all(d <= tol), (init, b, float((d / tol).max()))
            if not init:
                _check_vbound(res, b, res.Z[b], res.N[b], "1w-nuclear", f"nuclear[{b}]")


# ------------------------------------------------------------------------------------------------ four-wave kernel
IDS_4W = [c.name for c in R.CASES_4W]
PATHS_4W = {"jacobi": dict(zcert=False, tkeig=0), "zcert": dict(zcert=True, tkeig=0), "topk": dict(zcert=False, tkeig=1000),
            "zcert+topk": dict(zcert=True, tkeig=1000)}


@pytest.mark.parametrize("case", R.CASES_4W, ids=IDS_4W)
def test_four_wave(gpu, case):
    """r > 1: init form and iteration form (N = 0 on entry), cold and warm, zcert 0 / 1, tkeig on / off.  A step
    without a rescaling leaves N alone and sets nzero (the r-column stages keep N as exact zero)."""
    zp = _zp()
    refs = R.case_refs(case)
    X = case.X()
    rng = np.random.default_rng(3)
    Z0 = X + 0.05 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    Qw = np.stack([_eig_q(r.E, 1e-3, b) for b, r in enumerate(refs)])
    zero = np.zeros_like(X)
    for path, pk in PATHS_4W.items():
        res = zp.zprox_host(X, case.tx, case.rx, init=True, **_kw(case), **pk)
        for b, ref in enumerate(refs):
            _check_z(res.Z[b], ref, case.tx, f"{case.name}[{b}] init", "4w-" + path)
            _check_vbound(res, b, res.Z[b], zero[b], "4w-" + path, case.name)
        for warm in (False, True):
            tag = f"4w-{path}-{'warm' if warm else 'cold'}"
            res = zp.zprox_host(X, case.tx, case.rx, Z=Z0, mu=0.9, Q=Qw if warm else None, warm=warm, it=2,
                                last_res=1e300, **_kw(case), **pk)
            for b, ref in enumerate(refs):
                label = f"{case.name}[{b}] it"
                _check_z(res.Z[b], ref, case.tx, label, tag)
                if ref.any_fired:
                    assert res.nzero[b] == 0, label
                    _check_n(res, b, case, X, zero, np.full(case.batch, 0.9), ref, tag, label)
                    _check_vbound(res, b, res.Z[b], res.N[b], tag, label)
                else:
                    assert res.nzero[b] == 1 and not res.N[b].any(), label
                    _check_vbound(res, b, res.Z[b], zero[b], tag, label)
            assert np.all((res.status & ~ACE_ST_CONVERGED) == 0) and np.all(res.iters == 2)
        if pk["tkeig"]:
            assert res.tkcnt[1] == 0, (case.name, path, res.tkcnt)


@pytest.mark.parametrize("name", ["16x16-r2", "8x8-r5"])
def test_four_wave_with_n(gpu, refs_with_n, name):
    case = next(c for c in R.CASES_4W if c.name == name)
    X, Z0, N, mu, refs = refs_with_n[name]
    for path in ("jacobi", "zcert+topk"):
        res = _zp().zprox_host(X, case.tx, case.rx, Z=Z0, N=N, mu=mu, it=4, last_res=1e300, **_kw(case), **PATHS_4W[path])
        for b, ref in enumerate(refs):
            label = f"{name}[{b}] it N"
            if ref.any_fired:
                _check_z(res.Z[b], ref, case.tx, label, f"4w-{path}-N")
                _check_n(res, b, case, X, N, mu, ref, f"4w-{path}-N", label)
                _check_vbound(res, b, res.Z[b], res.N[b], f"4w-{path}-N", label)
            else:
                Zm = R.to_E(res.Z[b], case.tx)
                assert np.all(np.abs(Zm - ref.Z_hi) <= 2 * R.U * (np.abs(ref.Z_hi) + np.abs(R.to_E(N[b], case.tx)) / mu[b])), label
                assert res.nzero[b] == 1, label


# ------------------------------------------------------------------------------------------------ 3: certificates
def _cert_step(ka, kind, **kw):
    x = R.from_E(ka.E, 1)[None]
    Z0 = x.astype(np.complex64).astype(np.complex128)
    W = x - Z0
    assert np.array_equal(Z0 + W, x)
    return _zp().zprox_host(W, R.CERT_T, R.CERT_T, Z=Z0, nzero=1, Q=ka.Q[None], warm=True, wmode=True, pingpong=True,
                            mu=1.3, last_res=1e300, m=R.m_of(R.CERT_T, R.CERT_T, kind),
                            rank_one=1 if kind == "r1" else None, **kw)


@pytest.mark.parametrize("kind", R.CERT_KINDS)
@pytest.mark.parametrize("delta", R.CERT_DELTAS)
def test_certificate_soundness(gpu, kind, delta):
    """Top-group share f (1 +- delta) with the exact eigenvectors as the warm start: below the threshold the step
    rescales (and matches the known answer), above it (by more than the kernel's 1e-9 margin) Z' = E bit for bit.
    The lean kernel then takes the certified state: the same input is certified again, the partner below the
    threshold is not."""
    zp = _zp()
    rl, fl = R.profile_of(R.CERT_T, R.CERT_T, kind)
    above, below = R.cert_input(kind, delta), R.cert_input(kind, -delta)
    ra = _cert_step(above, kind, it=2)
    assert _bits_equal(R.to_E(ra.Z[0], 16), above.E) and ra.nzero[0] == 1 and ra.avok[0] == 1 and ra.kfok[0] == 1
    assert _sentinel(ra.N[0], zp.SENTINEL)
    vr = float(sum(sorted(above.lam, reverse=True)[: rl[0]]))
    assert ra.kf[0, 0] == pytest.approx(math.sqrt(vr), rel=1e-12)     # sqrt of the certified top-r sum

    ref_b = R.argmin_z_ref(below.E, rl, fl)
    assert ref_b.fired == [True]
    rb = _cert_step(below, kind, it=2)
    assert rb.kfok[0] == 0 and rb.nzero[0] == 0 and rb.avok[0] == 0
    assert not _bits_equal(R.to_E(rb.Z[0], 16), below.E)
    _check_z(rb.Z[0], ref_b, 16, f"cert {kind} -{delta:g}", "1w-cert")

    # the lean kernel on the certified state (kf, kfcum = 0, Q as the step left it), iteration 3
    state = dict(kf=ra.kf, kfcum=ra.kfcum, kfok=1, nzero=1, Q=ra.Q, warm=True, wmode=True, pingpong=True, lean=True,
                 it=3, mu=1.3, last_res=1e300, m=R.m_of(16, 16, kind), rank_one=1 if kind == "r1" else None)
    Za = ra.Z                                   # = E_above
    same = zp.zprox_host(np.zeros_like(Za), 16, 16, Z=Za, **state)
    assert same.zit[0] == 3 and _bits_equal(same.Z[0], Za[0]) and same.nzero[0] == 1 and same.avok[0] == 1
    assert _sentinel(same.N[0], zp.SENTINEL) and same.kfok[0] == 1
    Wb = R.from_E(below.E, 1)[None] - Za        # exact: both lie on one dyadic grid
    assert np.array_equal(Za + Wb, R.from_E(below.E, 1)[None])
    part = zp.zprox_host(Wb, 16, 16, Z=Za, **state)
    assert part.zit[0] != 3 and part.kfok[0] == 0 and part.nzero[0] == 0, "the lean kernel certified a rescaled step"
    _check_z(part.Z[0], ref_b, 16, f"lean {kind} -{delta:g}", "1w-lean")


# ------------------------------------------------------------------------------------------------ 5: iteration control
def test_iteration_control(gpu):
    """last_res, the mu update, ACE_ST_CONVERGED / done in both fixed_iters modes, iters and opt_X against the
    reference, on inputs whose comparisons are all at least 1e-6 (relative) from equality."""
    zp = _zp()
    case = R.CASES_1W[2]   # 8x8, N = 0
    refs = R.case_refs(case)
    X = case.X()
    rng = np.random.default_rng(12)
    Z0 = X + 0.02 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    mu = np.array([0.4, 0.9, 2.2])
    base = dict(obj2=2.5, nAX2=60.0, nY2=58.0, nJM2=0.7, dY2=0.3, dAtY=0.2, nAtY=44.0)
    scenarios = {
        "grow":      dict(tol_rel=1e-4, last_res=0.5, opt_obj=1.0),          # res_comb > 0.9 last_res: mu rho; not improved
        "keep":      dict(tol_rel=1e-4, last_res=1e3, opt_obj=9.0),          # no mu update; improved
        "converged": dict(tol_rel=10.0, last_res=0.5, opt_obj=9.0),          # every residual below its threshold
    }
    for sname, sc in scenarios.items():
        for fixed in (True, False):
            st = dict(base, last_res=sc["last_res"], opt_obj=sc["opt_obj"])
            res = zp.zprox_host(X, 8, 8, Z=Z0, mu=mu, it=7, fixed_iters=fixed, tol_rel=sc["tol_rel"], tol_abs=1e-8,
                                rho=1.03, **st, **_kw(case))
            for b, ref in enumerate(refs):
                Xe = R.to_E(X[b], 8)
                want = R.iter_control_ref(Xe, R.to_E(Z0[b], 8), ref, mu=mu[b], m=case.m(), n=64, r=1, st=st,
                                          tol_rel=sc["tol_rel"], tol_abs=1e-8, rho=1.03, fixed_iters=fixed)
                label = f"{sname} fixed={fixed} [{b}]"
                assert want["margin"] >= 1e-6, (label, want["margin"])
                assert want["conv"] == (sname == "converged"), label
                assert bool(res.status[b] & ACE_ST_CONVERGED) == want["conv"], label
                assert res.done[b] == int(want["done"]) and res.iters[b] == 7, label
                assert res.mu[b] == want["mu"], (label, res.mu[b], want["mu"])
                if want["done"]:
                    assert res.last_res[b] == sc["last_res"], label
                else:
                    assert res.last_res[b] == pytest.approx(want["last_res"], rel=1e-12), label
                assert want["improved"] == (sname != "grow"), label
                if want["improved"]:
                    assert res.opt_obj[b] == math.sqrt(2.5) and res.optsrc[b] == 0, label
                    assert _bits_equal(res.optX[b], X[b]), label
                else:
                    assert res.opt_obj[b] == sc["opt_obj"] and _sentinel(res.optX[b], zp.SENTINEL), label
    # wmode: an improved iterate of a certified realisation (N = 0, Z' = X) is left in the Z' buffer (optsrc)
    Xw, Zw, W = _wmode_inputs(case)
    Q = np.stack([_eig_q(r.E) for r in refs])
    res = zp.zprox_host(W, 8, 8, Z=Zw, nzero=1, Q=Q, warm=True, wmode=True, pingpong=True, it=7, mu=mu, last_res=1e3,
                        opt_obj=9.0, **base, **_kw(case))
    for b, ref in enumerate(refs):
        if ref.any_fired:
            assert res.optsrc[b] == 0 and _bits_equal(res.optX[b], Xw[b]), b
        else:
            assert res.optsrc[b] == 1 + (7 & 1) and _sentinel(res.optX[b], zp.SENTINEL), b
        assert res.opt_obj[b] == math.sqrt(2.5)


def test_iteration_control_four_wave(gpu):
    """The same comparison on the four-wave kernel (r = 5; it forms the dual terms from its Y and K Y buffers, zero
    here): last_res, the mu update, CONVERGED / done, iters, opt_X (all columns in row mode)."""
    zp = _zp()
    case = R.CASES_4W[1]   # 8x8-r5
    refs = R.case_refs(case)
    X = case.X()
    rng = np.random.default_rng(13)
    Z0 = X + 0.02 * (rng.standard_normal(X.shape) + 1j * rng.standard_normal(X.shape))
    mu = np.array([0.4, 0.9, 2.2])
    base = dict(obj2=2.5, nAX2=300.0, nY2=290.0, nJM2=0.7, dY2=0.3)
    for sname, sc in (("grow", dict(tol_rel=1e-4, last_res=0.5, opt_obj=1.0)),
                      ("keep", dict(tol_rel=1e-4, last_res=1e3, opt_obj=9.0)),
                      ("converged", dict(tol_rel=10.0, last_res=0.5, opt_obj=9.0))):
        for fixed in (True, False):
            st = dict(base, last_res=sc["last_res"], opt_obj=sc["opt_obj"])
            res = zp.zprox_host(X, 8, 8, Z=Z0, mu=mu, it=7, fixed_iters=fixed, tol_rel=sc["tol_rel"], tol_abs=1e-8,
                                rho=1.03, **st, **_kw(case))
            for b, ref in enumerate(refs):
                want = R.iter_control_ref(R.to_E(X[b], 8), R.to_E(Z0[b], 8), ref, mu=mu[b], m=case.m(), n=64, r=5,
                                          st=st, tol_rel=sc["tol_rel"], tol_abs=1e-8, rho=1.03, fixed_iters=fixed)
                label = f"4w {sname} fixed={fixed} [{b}]"
                assert want["margin"] >= 1e-6, (label, want["margin"])
                assert want["conv"] == (sname == "converged") and want["improved"] == (sname != "grow"), label
                assert bool(res.status[b] & ACE_ST_CONVERGED) == want["conv"], label
                assert res.done[b] == int(want["done"]) and res.iters[b] == 7, label
                assert res.mu[b] == want["mu"], (label, res.mu[b], want["mu"])
                if want["done"]:
                    assert res.last_res[b] == sc["last_res"], label
                else:
                    assert res.last_res[b] == pytest.approx(want["last_res"], rel=1e-12), label
                if want["improved"]:
                    assert res.opt_obj[b] == math.sqrt(2.5) and _bits_equal(res.optX[b], X[b]), label
                else:
                    assert res.opt_obj[b] == sc["opt_obj"] and _sentinel(res.optX[b], zp.SENTINEL), label


# ------------------------------------------------------------------------------------------------ 6: degenerate spectra
def test_degenerate_spectra(gpu):
    zp = _zp()
    for name, (ka, kind) in R.degenerate_inputs().items():
        rl, fl = R.profile_of(16, 16, kind)
        ref = R.argmin_z_ref(ka.E, rl, fl)
        x = R.from_E(ka.E, 1)[None]
        for path in ("jacobi", "topk"):
            res = zp.zprox_host(x, 16, 16, init=True, **PATHS_1W[path])
            Zm = R.to_E(res.Z[0], 16)
            assert np.all(np.isfinite(Zm.view(np.float64))) and math.isfinite(res.vbound[0]), (name, path)
            if name == "straddle":
                # lambda_3 = lambda_4 across the first boundary: Z depends on the basis chosen inside the tie; its
                # singular values sqrt(c_i lambda_i) do not
                sv = np.linalg.svd(Zm, compute_uv=False)
                np.testing.assert_allclose(sv, ref.singular_values(), rtol=1e-10, atol=0.0)
            else:
                _check_z(res.Z[0], ref, 16, f"degenerate {name}", "1w-" + path + "-degenerate")
        # iteration form (one-wave, cold and warm), and the four-wave kernel on the two-column iterate [E | E]:
        # E E^H doubles, so its Z is [Z | Z] of the same reference
        x2 = np.concatenate([x, x], axis=1)
        runs = [("1w-it-cold", zp.zprox_host(x, 16, 16, Z=0.9 * x, mu=0.7, it=1, last_res=1e300), 1),
                ("1w-it-warm", zp.zprox_host(x, 16, 16, Z=0.9 * x, mu=0.7, it=1, last_res=1e300, warm=True,
                                             Q=ka.Q[None], tkeig=1000), 1),
                ("4w-init", zp.zprox_host(x2, 16, 16, r=2, init=True), 2),
                ("4w-it-topk", zp.zprox_host(x2, 16, 16, r=2, Z=0.9 * x2, mu=0.7, it=1, last_res=1e300, tkeig=1000), 2)]
        for tag, res, r in runs:
            assert math.isfinite(res.vbound[0]) and (res.status[0] & ~ACE_ST_CONVERGED) == 0, (name, tag)
            for j in range(r):
                Zj = res.Z[0][j:j + 1]
                assert np.all(np.isfinite(Zj.view(np.float64))), (name, tag)
                if name == "straddle":
                    sv = np.linalg.svd(R.to_E(Zj, 16), compute_uv=False)
                    np.testing.assert_allclose(sv, ref.singular_values(), rtol=1e-10, atol=0.0)
                else:
                    _check_z(Zj, ref, 16, f"degenerate {name} col {j}", tag + "-degenerate")
    z = np.zeros((2, 1, 256), np.complex128)
    for kw in (dict(init=True), dict(Z=z, it=1, last_res=1e300), dict(init=True, tkeig=1000)):
        res = zp.zprox_host(z, 16, 16, **kw)
        assert not res.Z.any() and np.all(res.vbound == 0.0) and np.all((res.status & ~ACE_ST_CONVERGED) == 0)
    z2 = np.zeros((2, 2, 256), np.complex128)
    for kw in (dict(init=True), dict(Z=z2, it=1, last_res=1e300), dict(init=True, tkeig=1000, zcert=True)):
        res = zp.zprox_host(z2, 16, 16, r=2, **kw)
        assert not res.Z.any() and np.all(res.vbound == 0.0) and np.all((res.status & ~ACE_ST_CONVERGED) == 0)


# ---------------------------------------------------------------------------- 6: |E| near 1e+-100 on every eigensolver
@pytest.mark.parametrize("name", list(R.OUT_OF_BAND))
def test_out_of_band_magnitudes(gpu, name):
    """tr(E E^H) far outside [2^-400, 2^400], where the eigensolvers work on an exactly rescaled H (eig_prescale):
    the one-wave kernel's Jacobi, topk_tri (and its fallback to Jacobi on a clustered top group) and r1_top, init
    and warm iteration form; the four-wave kernel (jacobi_eig32, topk_tri on wave 0) on a two-column iterate
    [E0 | E0'], zcert 0, tkeig on and off, init, cold and warm iteration; the r-column nuclear prox, whose soft
    threshold reads jacobi_eig32's eigenvalues in absolute terms."""
    zp = _zp()
    e = R.OUT_OF_BAND[name]
    E0, E1 = R.out_of_band_pair(name)
    full, one = R.profile_of(16, 16, "full"), R.profile_of(16, 16, "r1")
    x = R.from_E(E0, 1)[None]
    # ---- one-wave kernel
    for tag, prof, kw in (("jacobi", full, dict()), ("topk", full, dict(tkeig=1000)),
                          ("r1lz", one, dict(rank_one=1, r1lz=True)), ("r1-jacobi", one, dict(rank_one=1))):
        ref = R.argmin_z_ref(E0, *prof)
        assert ref.any_fired and ref.margin >= 1e-6 and ref.gap >= 1e-3
        res = zp.zprox_host(x, 16, 16, init=True, **kw)
        _check_z(res.Z[0], ref, 16, f"{name} init", f"1w-{tag}-outofband")
        _check_vbound(res, 0, res.Z[0], np.zeros_like(x[0]), f"1w-{tag}-outofband", name)
        if tag == "topk":
            assert res.tkcnt.tolist() == [1, 0], res.tkcnt
        res = zp.zprox_host(x, 16, 16, Z=0.9 * x, mu=0.9, it=2, last_res=1e300, warm=True, Q=_eig_q(E0, 1e-3)[None], **kw)
        _check_z(res.Z[0], ref, 16, f"{name} warm", f"1w-{tag}-outofband")
        _check_n(res, 0, R.Case("oob", 16, 16, 1, "full", (1,), (0.0,), 0), x, np.zeros_like(x), np.array([0.9]), ref,
                 f"1w-{tag}-outofband", name)
        _check_vbound(res, 0, res.Z[0], res.N[0], f"1w-{tag}-outofband", name)
        assert (res.status[0] & ~ACE_ST_CONVERGED) == 0
    # a clustered top group makes topk_tri decline: the fallback rebuilds H (and rescales it again) for Jacobi;
    # the counters are those of the same input inside the band
    tri = R.degenerate_inputs()["triple"][0].E
    ref = R.argmin_z_ref(tri, *full)
    inband = zp.zprox_host(R.from_E(tri, 1)[None], 16, 16, init=True, tkeig=1000)
    tri_s = np.ldexp(tri.real, e) + 1j * np.ldexp(tri.imag, e)
    res = zp.zprox_host(R.from_E(tri_s, 1)[None], 16, 16, init=True, tkeig=1000)
    print(f"  triple top eigenvalue: tkcnt in band {inband.tkcnt.tolist()}, out of band {res.tkcnt.tolist()}")
    assert res.tkcnt.tolist() == inband.tkcnt.tolist()
    Zs = R.to_E(res.Z[0], 16)
    back = np.ldexp(Zs.real, -e) + 1j * np.ldexp(Zs.imag, -e)          # exact
    assert ref.err(back) <= ref.tol
    _note("1w-topk-fallback-outofband", ref.err(back) / ref.tol)
    # ---- four-wave kernel, r = 2
    E2 = np.hstack([E0, E1])
    x2 = R.from_E(E2, 2)[None]
    ref2 = R.argmin_z_ref(E2, *full)
    assert ref2.any_fired and ref2.margin >= 1e-6 and ref2.gap >= 1e-3
    case2 = R.Case("oob2", 16, 16, 2, "full", (1,), (0.0,), 0)
    for tk in (0, 1000):
        tag = f"4w-{'topk' if tk else 'jacobi'}-outofband"
        res = zp.zprox_host(x2, 16, 16, r=2, init=True, zcert=False, tkeig=tk)
        _check_z(res.Z[0], ref2, 16, f"{name} r=2 init", tag)
        _check_vbound(res, 0, res.Z[0], np.zeros_like(x2[0]), tag, name)
        if tk:
            assert res.tkcnt.tolist() == [1, 0], res.tkcnt
        for warm in (False, True):
            res = zp.zprox_host(x2, 16, 16, r=2, Z=0.9 * x2, mu=0.9, it=2, last_res=1e300, zcert=False, tkeig=tk,
                                warm=warm, Q=_eig_q(E2, 1e-3)[None] if warm else None)
            _check_z(res.Z[0], ref2, 16, f"{name} r=2 it warm={warm}", tag)
            _check_n(res, 0, case2, x2, np.zeros_like(x2), np.array([0.9]), ref2, tag, name)
            _check_vbound(res, 0, res.Z[0], res.N[0], tag, name)
            assert (res.status[0] & ~ACE_ST_CONVERGED) == 0 and res.nzero[0] == 0
    # ---- nuclear prox at r = 2 (jacobi_eig32 on the 2 x 2 Gram matrix): Z = U soft(S, 1/mu) V^H is homogeneous,
    # Z(c E, c tau) = c Z(E, tau), so the reference is numpy's SVD of the unscaled problem times 2^e (exact).
    # Through the Gram matrix sigma_i carries u kappa sigma_1 and V u / (1 - kappa^-2); with the products and the
    # threshold: || Z - Z* ||_F <= 16 u (kappa + 1 / (1 - kappa^-2) + 4) || E ||_F, kappa = sigma_1 / sigma_2 = 2
    rng = np.random.default_rng(8)
    qa = np.linalg.qr(rng.standard_normal((256, 2)) + 1j * rng.standard_normal((256, 2)))[0]
    qb = np.linalg.qr(rng.standard_normal((2, 2)) + 1j * rng.standard_normal((2, 2)))[0]
    Eb = (qa * np.array([1.0, 0.5])[None, :]) @ qb.conj().T           # n x r, singular values 1, 1/2
    tau = 0.125
    Ub, Sb, Vb = np.linalg.svd(Eb, full_matrices=False)
    Zb = (Ub * np.maximum(0.0, Sb - tau)[None, :]) @ Vb
    Xs = np.ldexp(Eb.real, e) + 1j * np.ldexp(Eb.imag, e)
    xs = np.ascontiguousarray(Xs.T)[None]                             # [1][r][n]
    res = zp.zprox_host(xs, 16, 16, variant="A2nuclear", r=2, Z=0.9 * xs, mu=math.ldexp(1.0 / tau, -e), it=1,
                        last_res=1e300)
    got = res.Z[0].T
    got = np.ldexp(got.real, -e) + 1j * np.ldexp(got.imag, -e)
    err, tol = np.linalg.norm(got - Zb), 16 * R.U * (2 + 1 / 0.75 + 4) * np.linalg.norm(Eb)
    _note("4w-nuclear-outofband", err / tol)
    assert np.all(np.isfinite(res.Z.view(np.float64))) and err <= tol, (name, err, tol)


def test_subnormal_trace_stays_finite(gpu):
    """|E| about 1e-156: E E^H is subnormal (its entries keep a few bits), the prescale factor is clamped to a finite
    power of two, and Z' stays finite on both kernels."""
    E0 = R.out_of_band_pair("tiny")[0]
    Es = np.ldexp(E0.real, -198) + 1j * np.ldexp(E0.imag, -198)       # 2^-530 in all
    x = R.from_E(Es, 1)[None]
    for kw in (dict(), dict(tkeig=1000), dict(rank_one=1, r1lz=True)):
        res = _zp().zprox_host(x, 16, 16, init=True, **kw)
        assert np.all(np.isfinite(res.Z.view(np.float64))) and math.isfinite(res.vbound[0]), kw
    x2 = np.concatenate([x, x], axis=1)
    for kw in (dict(), dict(tkeig=1000)):
        res = _zp().zprox_host(x2, 16, 16, r=2, init=True, **kw)
        assert np.all(np.isfinite(res.Z.view(np.float64))) and math.isfinite(res.vbound[0]), kw


# ------------------------------------------------------------------------------------------------ 4: non-finite input
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_vbound_nan_for_non_finite_input(gpu, bad):
    case = R.CASES_1W[2]
    X = case.X()
    X[1, 0, 17] = bad
    Z0 = case.X()
    good = _zp().zprox_host(case.X(), 8, 8, Z=Z0, it=1, last_res=1e300, **_kw(case))
    for kw in (dict(init=True), dict(Z=Z0, it=1, last_res=1e300),
               dict(Z=Z0, nzero=1, wmode=True, pingpong=True, it=1, last_res=1e300)):
        res = _zp().zprox_host(X, 8, 8, **kw, **_kw(case))
        assert math.isnan(res.vbound[1]), kw
        assert np.all(np.isfinite(res.vbound[[0, 2]])), kw
    res = _zp().zprox_host(X, 8, 8, Z=Z0, it=1, last_res=1e300, **_kw(case))
    for b in (0, 2):     # the neighbours are what they are without the bad realisation
        assert _bits_equal(res.Z[b], good.Z[b]) and res.vbound[b] == good.vbound[b]
    r4 = R.CASES_4W[1]
    X4 = r4.X()
    X4[2, 3, 5] = bad
    res = _zp().zprox_host(X4, 8, 8, Z=r4.X(), it=1, last_res=1e300, **_kw(r4))
    assert math.isnan(res.vbound[2]) and np.all(np.isfinite(res.vbound[:2]))


# ------------------------------------------------------------------------------------------------ 7: untouched memory
def test_done_realisations_are_left_alone(gpu):
    zp = _zp()
    case = R.CASES_1W[2]
    X, Z0, N, mu = _iter_inputs(case, 5)
    done = np.array([0, 1, 0], np.int32)
    res = zp.zprox_host(X, 8, 8, Z=Z0, N=N, mu=mu, done=done, it=9, last_res=0.25, opt_obj=1e9, obj2=1.0, **_kw(case))
    assert _bits_equal(res.Z[1], Z0[1]) and _bits_equal(res.N[1], N[1])      # in place: the inputs stand
    assert _sentinel(res.optX[1], zp.SENTINEL) and res.iters[1] == 0 and res.mu[1] == mu[1] and res.last_res[1] == 0.25
    assert not _bits_equal(res.Z[0], Z0[0]) and res.iters[0] == 9 and _bits_equal(res.optX[0], X[0])
    Xw, Zw, W = _wmode_inputs(case)
    for lean in (False, True):
        res = zp.zprox_host(W, 8, 8, Z=Zw, nzero=1, done=done, Q=np.stack([np.eye(8)] * 3), warm=True, wmode=True,
                            pingpong=True, lean=lean, kfok=1, kf=np.ones(4), it=9, last_res=0.25, **_kw(case))
        assert _sentinel(res.Z[1], zp.SENTINEL) and _sentinel(res.N[1], zp.SENTINEL), lean   # ping-pong: never written
        assert _sentinel(res.optX[1], zp.SENTINEL) and _sentinel(res.Xcur[1], zp.SENTINEL), lean
        assert res.iters[1] == 0 and res.vbound[1] == 0.0 and res.zit[1] == 0, lean
        assert not _sentinel(res.Z[0], zp.SENTINEL), lean
    r4 = R.CASES_4W[1]
    X4 = r4.X()
    res = zp.zprox_host(X4, 8, 8, Z=X4 * 0.5, done=done, it=2, last_res=0.25, **_kw(r4))
    assert _bits_equal(res.Z[1], X4[1] * 0.5) and res.iters[1] == 0 and res.iters[0] == 2


def test_batch_of_65_and_position_invariance(gpu):
    """65 realisations with their own spectra (ragged groups of 4 and 8) against their references, on the in-place
    path and through the lean kernel; realisation 0 alone equals its slot in the batch bit for bit."""
    zp = _zp()
    case = R.CASE_B65
    refs = R.case_refs(case)
    X, Z0, N, mu = _iter_inputs(case, 31, with_n=False)
    kw = dict(Z=Z0, mu=mu, it=4, last_res=1e300, **_kw(case))
    res = zp.zprox_host(X, 8, 8, **kw)
    for b, ref in enumerate(refs):
        _check_z(res.Z[b], ref, 8, f"b65[{b}]", "1w-jacobi-b65")
        _check_vbound(res, b, res.Z[b], res.N[b], "1w-jacobi-b65", f"b65[{b}]")
    for b in (0, 64):
        one = zp.zprox_host(X[b:b + 1], 8, 8, **dict(kw, Z=Z0[b:b + 1], mu=mu[b:b + 1]))
        assert _bits_equal(one.Z[0], res.Z[b]) and _bits_equal(one.N[0], res.N[b]) and one.vbound[0] == res.vbound[b]
        assert one.last_res[0] == res.last_res[b] and one.mu[0] == res.mu[b]
    # wmode + lean: a certified step first (warm start = the eigenvectors), then the lean kernel on its state
    Xw, Zw, W = _wmode_inputs(case)
    Q = np.stack([_eig_q(r.E) for r in refs])
    wk = dict(warm=True, wmode=True, pingpong=True, mu=0.7, last_res=1e300, **_kw(case))
    s1 = zp.zprox_host(W, 8, 8, Z=Zw, nzero=1, Q=Q, it=2, **wk)
    for b, ref in enumerate(refs):
        _check_z(s1.Z[b], ref, 8, f"b65[{b}] wmode", "1w-jacobi-wmode-b65")
        assert s1.kfok[b] == (0 if ref.any_fired else 1), b
    # second step from the first one's outputs: W = 0, so E = Z' of step 1; certified realisations stay
    # certified through the lean kernel (zit = it), the others run the full kernel again
    s2 = zp.zprox_host(np.zeros_like(W), 8, 8, Z=s1.Z, N=np.where(s1.nzero[:, None, None] == 1, 0.0, s1.N),
                       nzero=s1.nzero, kfok=s1.kfok, kf=s1.kf, kfcum=s1.kfcum, Q=s1.Q, lean=True, it=3, **wk)
    for b, ref in enumerate(refs):
        if not ref.any_fired:
            assert s2.zit[b] == 3 and _bits_equal(s2.Z[b], s1.Z[b]) and s2.nzero[b] == 1 and s2.avok[b] == 1, b
        else:
            assert s2.zit[b] == 0, b
        assert np.all(np.isfinite(s2.Z[b].view(np.float64)))
    one = zp.zprox_host(np.zeros_like(W[64:65]), 8, 8, Z=s1.Z[64:65],
                        N=np.where(s1.nzero[64:65, None, None] == 1, 0.0, s1.N[64:65]), nzero=s1.nzero[64:65],
                        kfok=s1.kfok[64:65], kf=s1.kf[64:65], kfcum=s1.kfcum[64:65], Q=s1.Q[64:65], lean=True, it=3, **wk)
    assert _bits_equal(one.Z[0], s2.Z[64]) and one.vbound[0] == s2.vbound[64] and one.zit[0] == s2.zit[64]


def test_explicit_profile_equals_derived(gpu):
    """The profile given entry by entry runs as the one the entry derives from m."""
    case = R.CASES_1W[3]
    X = case.X()
    a = _zp().zprox_host(X, 16, 16, init=True, **_kw(case))
    b = _zp().zprox_host(X, 16, 16, init=True, profile=case.profile(), m=5)
    assert _bits_equal(a.Z, b.Z)


def test_unsupported_combinations(gpu):
    from ace_amd import AceError
    X = R.CASES_1W[2].X()
    for kw in (dict(wmode=True), dict(pingpong=True), dict(wmode=True, pingpong=True, init=True),
               dict(lean=True, wmode=True, pingpong=True, Z=X), dict(lean=True, wmode=True, pingpong=True, warm=True,
                                                                    Q=np.stack([np.eye(8)] * 3), variant="A2nuclear")):
        with pytest.raises(AceError) as e:
            _zp().zprox_host(X, 8, 8, **kw)
        assert e.value.code == -2, kw
    with pytest.raises(AceError) as e:
        _zp().zprox_host(X[:, :, :63].copy().reshape(3, 1, 63), 7, 9)     # odd tx: the API pads it, the kernels decline
    assert e.value.code == -2
