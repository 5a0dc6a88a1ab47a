"""CPU self-test of tests/zprox_ref.py, the reference of the Z-step suite (tests/test_gpu_zprox.py).

* the general reference (mpmath eigensolver) and the known-answer construction (no eigensolver) agree to 1e-30;
* every input of the GPU suite shows, on the reference alone, the firing pattern it was built for, decisions
  at least 1e-6 and scale-changing boundaries at least 1e-3 (relative) away from a tie;
* the f64 oracle (LAPACK) is inside the tolerance on every such input; the largest err / (u kappa) it reaches
  is printed and is zprox_ref.ORACLE_RATIO (to within a quarter), from which the kernels' multiplier is 8 x;
* numpy models of a wrong Z-step land at least 10 x outside the tolerance on every input where a rescaling
  fires and the fault changes the factors applied (a missing tie-break needs tied clamped eigenvalues, a stale
  spectrum a second profile entry): this keeps the tolerance from being loose enough to hide such an error.
"""
import math

import mpmath as mp
import numpy as np
import pytest

import ace_oracle as O
import zprox_ref as R


def _mp_diff(Za, Zb):
    with mp.workdps(R.DPS):
        d = max(abs(Za[i, j] - Zb[i, j]) for i in range(Za.rows) for j in range(Za.cols))
        n = max(abs(Zb[i, j]) for i in range(Zb.rows) for j in range(Zb.cols))
        return float(d / n) if n > 0 else float(d)


KA_SHAPES = [(4, 4), (8, 8), (16, 16), (16, 8), (8, 32)]


@pytest.mark.parametrize("tx,rx", KA_SHAPES, ids=[f"{a}x{b}" for a, b in KA_SHAPES])
def test_general_reference_equals_known_answer(tx, rx):
    worst = 0.0
    for kind in ("full", "m3n", "r1"):
        rl, fl = R.profile_of(tx, rx, kind)
        s = [1000 - 61 * i for i in range(min(tx, rx))]
        ka = R.known_answer(tx, rx, s, seed=3 + tx)
        H = ka.E @ ka.E.conj().T
        lam = sorted((float(v) for v in ka.lam), reverse=True)
        assert np.abs(np.sort(np.linalg.eigvalsh(H))[::-1] - lam).max() <= 64 * R.U * lam[0]
        assert np.abs(H @ ka.Q - ka.Q * np.array([float(v) for v in ka.lam])[None, :]).max() <= 64 * R.U * lam[0]
        Zk, _, fired_k, _ = R.known_answer_z(ka, rl, fl)
        ref = R.argmin_z_ref(ka.E, rl, fl)
        assert ref.fired == fired_k
        worst = max(worst, _mp_diff(R.ref_z_mp(ref), Zk))
    print(f"  {tx}x{rx}: max |Z_general - Z_known| / max|Z| = {worst:.2e}")
    assert worst <= 1e-30


def test_known_answer_suite_inputs():
    """The certificate pairs sit at f (1 +- delta) to within 1 % of delta; the well-posed degenerate inputs agree
    between the two constructions, the straddling tie does not have to (Z is ill-posed there)."""
    for kind in R.CERT_KINDS:
        rl, fl = R.profile_of(R.CERT_T, R.CERT_T, kind)
        for d in R.CERT_DELTAS:
            for sg in (1, -1):
                ka = R.cert_input(kind, sg * d)
                real = float(R.top_share(ka, rl[0]) / R.Fraction(fl[0]) - 1)
                assert abs(real - sg * d) <= 0.01 * d, (kind, sg * d, real)
                _, _, fired, _ = R.known_answer_z(ka, rl, fl)
                assert fired == [sg < 0]
    for name, (ka, kind) in R.degenerate_inputs().items():
        rl, fl = R.profile_of(16, 16, kind)
        Zk, _, fired_k, _ = R.known_answer_z(ka, rl, fl)
        ref = R.argmin_z_ref(ka.E, rl, fl)
        assert ref.fired == fired_k
        if name == "straddle":
            assert math.isinf(ref.kappa) or ref.kappa > 1e30
            sv = sorted((math.sqrt(float(c * l)) for c, l in zip(R.known_answer_z(ka, rl, fl)[1], ka.lam)), reverse=True)
            np.testing.assert_allclose(ref.singular_values(), sv, rtol=1e-14, atol=1e-14 * sv[0])
        else:
            assert _mp_diff(R.ref_z_mp(ref), Zk) <= 1e-30, name


@pytest.fixture(scope="module")
def suite():
    """(label, E, rl, fl, m, ZRef) of every general input of the GPU suite, references computed once."""
    out = []
    for case in R.ALL_CASES:
        rl, fl = case.profile()
        X = case.X()
        for b, ref in enumerate(R.case_refs(case)):
            out.append((f"{case.name}[{b}]", R.to_E(X[b], case.tx), rl, fl, case, ref))
    return out


def test_suite_patterns(suite):
    for case in R.ALL_CASES:
        refs = R.case_refs(case)
        pats = tuple(R.pattern(r) for r in refs)
        if case.want:
            assert pats == case.want, (case.name, pats)
        for b, r in enumerate(refs):
            assert r.margin >= 1e-6, (case.name, b, r.margin)
            if r.any_fired:
                assert r.gap >= 1e-3, (case.name, b, r.gap)
    b65 = [R.pattern(r) for r in R.case_refs(R.CASE_B65)]
    assert b65.count("none") >= 8 and b65.count("all") >= 8


def _oracle_z(E, case):
    tx, rx, r = case.tx, case.rx, case.r
    X = R.from_E(E, r).T.copy()    # n x r, as the oracle takes it
    Z = O.argmin_z_lowrank(X, np.zeros_like(X), 1.0, tx, rx, case.m(), case.n, 1 if case.kind == "r1" else 0)
    return R.to_E(Z.T, tx)


def test_oracle_inside_tolerance(suite):
    worst, where = 0.0, None
    for label, E, rl, fl, case, ref in suite:
        Zo = _oracle_z(E, case)
        if not ref.any_fired:
            assert np.array_equal(Zo, E), label
            continue
        ratio = ref.err(Zo) / (R.U * ref.kappa)
        if ratio > worst:
            worst, where = ratio, label
        assert ref.err(Zo) <= ref.tol, (label, ratio)
    # the known-answer inputs the GPU suite compares in full
    for name, (ka, kind) in R.degenerate_inputs().items():
        if name == "straddle":
            continue
        rl, fl = R.profile_of(16, 16, kind)
        ref = R.argmin_z_ref(ka.E, rl, fl)
        Zo = R.z_model(ka.E, rl, fl)[0]
        if ref.any_fired:
            ratio = ref.err(Zo) / (R.U * ref.kappa)
            if ratio > worst:
                worst, where = ratio, name
    print(f"  f64 oracle: max err / (u kappa) = {worst:.3f} at {where}; ORACLE_RATIO {R.ORACLE_RATIO}, "
          f"kernel multiplier {R.TOL_MULT}")
    # ORACLE_RATIO is this measurement with one LAPACK build; another may round differently, but not by a quarter
    assert worst <= 1.25 * R.ORACLE_RATIO


@pytest.mark.parametrize("kind", R.MUTANTS)
def test_wrong_models_land_outside(suite, kind):
    """Every input where a rescaling fires and the fault applies: the wrong model is >= 10 x the tolerance out."""
    extra = []
    # tied clamped eigenvalues with a rescaling: a rank-2 signal (gains 1, 1/2) without noise under the rank-one
    # profile
    for seed in (1, 2):
        E = R.lowrank_noise(16, 16, 2, 0.0, 900 + seed)
        rl, fl = R.profile_of(16, 16, "r1")
        extra.append((f"rank2[{seed}]", E, rl, fl, None, None))
    hit, least = 0, math.inf
    for label, E, rl, fl, case, ref in list(suite) + extra:
        _, sc_right = R.z_model(E, rl, fl)
        Zw, sc_wrong = R.z_model(E, rl, fl, kind)
        if not R.model_applies(kind, sc_right, sc_wrong):
            continue
        if ref is None:
            ref = R.argmin_z_ref(E, rl, fl)
        assert ref.any_fired
        hit += 1
        out = ref.err(Zw) / ref.tol
        least = min(least, out)
        assert out >= 10.0, (kind, label, out)
    print(f"  {kind}: {hit} inputs, closest err / tol = {least:.3g}")
    assert hit >= 2, kind


def test_iter_control_ref_against_f64():
    """The extended-precision control agrees with the plain f64 evaluation of the same formulas (:364-381)."""
    rng = np.random.default_rng(5)
    tx = rx = 8
    case = R.CASES_1W[2]
    rl, fl = case.profile()
    E = R.to_E(case.X()[1], tx)
    ref = R.case_refs(case)[1]
    Z0 = E + 0.01 * (rng.standard_normal(E.shape) + 1j * rng.standard_normal(E.shape))
    st = dict(obj2=3.0, nAX2=50.0, nY2=49.0, nJM2=0.3, dY2=0.2, dAtY=0.4, nAtY=40.0, opt_obj=2.0, last_res=1.0)
    out = R.iter_control_ref(E, Z0, ref, mu=0.7, m=64, n=64, r=1, st=st, tol_rel=1e-3, tol_abs=1e-4, rho=1.05,
                             fixed_iters=True)
    Z = ref.Z_hi
    jn2, dZ2 = np.linalg.norm(E - Z) ** 2, np.linalg.norm(Z - Z0) ** 2
    res_prim = math.sqrt(0.3 + jn2)
    res_comb = math.sqrt(res_prim ** 2 + 0.2 + dZ2)
    assert out["res_comb"] == pytest.approx(res_comb, rel=1e-13)
    assert out["res_dual"] == pytest.approx(0.7 * math.sqrt(0.4 + dZ2), rel=1e-13)
    assert out["improved"] and out["opt_obj"] == pytest.approx(math.sqrt(3.0), rel=1e-15)
    assert out["grow"] == (res_comb > 0.9) and out["mu"] == (0.7 * 1.05 if out["grow"] else 0.7)
    assert not out["done"] and out["last_res"] == pytest.approx(res_comb, rel=1e-13)


def test_entry_argument_errors():
    """ace_zprox_host checks its arguments before any device work: ACE_ERR_ARG (-1) for bad shapes and missing
    arrays, ACE_ERR_UNSUPPORTED (-2) for combinations no solve makes."""
    from ace_amd import AceError, zprox
    X = np.zeros((2, 1, 64), np.complex128)
    bad = [(dict(tx=8, rx=8, it=0), -1), (dict(tx=8, rx=8, warm=True), -1), (dict(tx=8, rx=8, rho=0.0), -1),
           (dict(tx=8, rx=8, profile=([9], [0.9])), -1), (dict(tx=8, rx=8, profile=([3], [1.5])), -1),
           (dict(tx=8, rx=8, m=5000), -1),
           (dict(tx=8, rx=8, wmode=True), -2), (dict(tx=8, rx=8, pingpong=True), -2),
           (dict(tx=8, rx=8, wmode=True, pingpong=True, init=True), -2),
           (dict(tx=8, rx=8, wmode=True, pingpong=True, lean=True), -2)]
    for kw, code in bad:
        kw = dict(kw)
        tx, rx = kw.pop("tx"), kw.pop("rx")
        with pytest.raises(AceError) as e:
            zprox.zprox_host(X, tx, rx, **kw)
        assert e.value.code == code, (kw, e.value)
    with pytest.raises(AceError) as e:
        zprox.zprox_host(np.zeros((1, 1, 63), np.complex128), 7, 9)
    assert e.value.code == -2
    with pytest.raises(AceError) as e:
        zprox.zprox_host(np.zeros((1, 1, 66), np.complex128), 2, 33)
    assert e.value.code == -1
