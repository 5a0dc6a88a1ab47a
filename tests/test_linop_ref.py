"""CPU self-test of tests/linop_ref.py: the exact reference honours its own tolerances, and the tolerances are
sharp enough to see a lost digit plane or a wrong exponent (no GPU)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import linop_ref as R

SHAPES = [(15, 33), (64, 256)]
KINDS = ["synth", "off", "pmj1", "pmj"]


def test_exact_matvec_equals_rational_arithmetic():
    rng = np.random.default_rng(1)
    E = rng.standard_normal((6, 10)) * np.exp(rng.uniform(-15, 15, (6, 10)))
    V = rng.standard_normal((3, 10)) * np.exp(rng.uniform(-15, 15, (3, 10)))
    V[1, 3] = 0.0
    c = 1.0 / math.sqrt(7.0)
    hi, lo = R.exact_matvec(E, V, c)
    for j in range(3):
        for i in range(6):
            ex = sum(Fraction(E[i, k]) * Fraction(V[j, k]) for k in range(10)) * Fraction(c)
            d = ex - Fraction(hi[j, i]) - Fraction(lo[j, i])
            assert abs(d) <= abs(ex) * Fraction(1, 2 ** 100)
    # an integer product is reproduced exactly by hi alone
    Ei = rng.integers(-1, 2, (8, 40)).astype(np.float64)
    Vi = rng.integers(-2 ** 20, 2 ** 20, (5, 40)).astype(np.float64)
    hi, lo = R.exact_matvec(Ei, Vi)
    assert np.array_equal(hi, (Vi.astype(np.int64) @ Ei.astype(np.int64).T).astype(np.float64)) and not lo.any()


def test_fma_ref_is_one_rounding_of_the_exact_value():
    rng = np.random.default_rng(2)
    Z, N = R.rand_vectors(rng, 3, 5), R.rand_vectors(rng, 3, 5)
    imu = 1.0 / np.array([0.7, 3.0, 1e-3])
    V = R.fma_ref(N, imu, Z).view(np.float64)
    Zr, Nr = Z.view(np.float64), N.view(np.float64)
    for j in range(3):
        for k in range(10):
            ex = Fraction(Zr[j, k]) - Fraction(Nr[j, k]) * Fraction(imu[j])
            assert V[j, k] == float(ex)
    assert np.array_equal(R.fma_ref(np.zeros_like(Z), imu, Z), Z)


def _recipes(rng, nv, k):
    """(name, vectors, bound) of every data recipe of the GPU tests."""
    out = []
    Vi = R.int_vectors(rng, nv, k)
    out.append(("integer", Vi, R.maxabs_rows(Vi)))
    Vf = R.rand_vectors(rng, nv, k)
    out.append(("random", Vf, R.maxabs_rows(Vf)))
    Ve = R.edge_vectors(rng, nv, k)
    out.append(("edges", Ve, R.maxabs_rows(Ve)))
    out.append(("loose", Vf, 1024.0 * R.maxabs_rows(Vf)))
    out.append(("zero", np.zeros_like(Vf), np.zeros(nv)))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", SHAPES)
def test_digit_model_is_inside_the_int8_tolerance(m, n, kind):
    rng = np.random.default_rng([m, n])
    A = R.codebook(kind, m, n)
    c, P, Q = R.phase_parts(A)
    Kr, Ki = R.kint(A)
    ops = [("A", R.real_expand(P + 1j * Q), c, n), ("AH", R.real_expand((P + 1j * Q).conj().T), c, m),
           ("K", R.real_expand(Kr + 1j * Ki), c * c, m)]
    for name, Ei, scale, k in ops:
        nnz = np.abs(Ei).sum(axis=1)
        if name != "K":
            assert nnz.max() <= (2 * k if kind.startswith("pmj") else k)
        for rname, V, bound in _recipes(rng, 8, k):
            e = R.kernel_exp(bound)
            hi, lo = R.exact_matvec(Ei, V.view(np.float64), scale)
            tol = R.i8_tol(Ei, scale, e, hi)
            out = R.digit_model(Ei, scale, V.view(np.float64), e).view(np.complex128)
            err = R.err_against(out, hi, lo)
            assert (err <= tol).all(), (name, rname, float((err / tol)[tol > 0].max()))
            if rname == "integer" and scale == 1.0:
                assert not err.any()
            if rname == "zero":
                assert not out.view(np.float64).any()


@pytest.mark.parametrize("m,n", SHAPES)
def test_wrong_digit_models_fall_outside_the_tolerance(m, n):
    """A lost lowest digit plane and a wrong exponent must show.  The digit image is 56 bits for a 55-bit
    nominal range, so an exponent one too low in both the cut and the scale is still exact (it is not a fault
    of the scheme); one too low in the scale alone, or two too low in both (the image wraps), are faults."""
    rng = np.random.default_rng([m, n, 7])
    A = R.codebook("synth", m, n)
    c, P, Q = R.phase_parts(A)
    Ei = R.real_expand(P + 1j * Q)
    V = R.rand_vectors(rng, 32, n, spread=0.0)
    for bound in (R.maxabs_rows(V), 1024.0 * R.maxabs_rows(V)):
        e = R.kernel_exp(bound)
        hi, lo = R.exact_matvec(Ei, V.view(np.float64), c)
        tol = R.i8_tol(Ei, c, e, hi)

        def worst(**kw):
            out = R.digit_model(Ei, c, V.view(np.float64), e, **kw).view(np.complex128)
            return float((R.err_against(out, hi, lo) / tol).max())
        good, dropped, scale_off = worst(), worst(drop_low=True), worst(scale_shift=-1)
        print(f"(m, n) = ({m}, {n}), bound / max|v| = {bound[0] / R.maxabs_rows(V)[0]:g}: max err / tol correct "
              f"{good:.3g}, lowest plane dropped {dropped:.3g}, scale exponent one low {scale_off:.3g}")
        assert good <= 1.0
        assert dropped > 4.0
        assert scale_off > 1e6
        assert worst(cut_shift=-1) <= 1.0
    e = R.kernel_exp(R.maxabs_rows(V))
    hi, lo = R.exact_matvec(Ei, V.view(np.float64), c)
    out = R.digit_model(Ei, c, V.view(np.float64), e, cut_shift=-2).view(np.complex128)
    assert float((R.err_against(out, hi, lo) / R.i8_tol(Ei, c, e, hi)).max()) > 1e6


@pytest.mark.parametrize("m,n", SHAPES)
def test_loose_bound_rms_of_the_model(m, n):
    """With vbound = 2^10 max|v| every component is rounded at 2^(e - 54): the error's RMS is the uniform-
    rounding value c sqrt(N_nz / 12) 2^(e - 54) (the GPU test's cap is 1.25 times it)."""
    rng = np.random.default_rng([m, n, 11])
    A = R.codebook("synth", m, n)
    c, P, Q = R.phase_parts(A)
    Ei = R.real_expand(P + 1j * Q)
    V = R.rand_vectors(rng, 40, n, spread=0.0)
    e = R.kernel_exp(1024.0 * R.maxabs_rows(V))
    hi, lo = R.exact_matvec(Ei, V.view(np.float64), c)
    out = R.digit_model(Ei, c, V.view(np.float64), e).view(np.complex128)
    err = R.err_against(out, hi, lo)
    assert err.size >= 1000
    ratio = float(np.sqrt(np.mean((err / R.uniform_rms(Ei, c, e)) ** 2)))
    print(f"(m, n) = ({m}, {n}): loose-bound error RMS / uniform-rounding value = {ratio:.3f}")
    assert 0.8 <= ratio <= 1.15


@pytest.mark.parametrize("M,K", [(15, 33), (64, 256), (33, 100)])
def test_3m_emulation_is_inside_the_gemm_tolerance(M, K):
    rng = np.random.default_rng([M, K])
    A = R.rand_vectors(rng, M, K, spread=2.0)
    V = R.rand_vectors(rng, 9, K)
    E = R.rand_vectors(rng, 9, M)
    Ah = R.rand_vectors(rng, K, M, spread=2.0)   # applied as Ah^H (M x K)
    for herm, Am in ((False, A), (True, Ah)):
        h, l = R.exact_cmatvec(Am, V, herm=herm)
        acc = R.gemm3m_model(Am, V, herm=herm)
        for sign, C in ((1, E + acc), (-1, E - acc)):
            err = R.err_against(C, h, l, add=E, sign=sign)
            tol = R.gemm_tol(Am, V, E=E, C=C, herm=herm)
            assert (err <= tol).all(), float((err / tol).max())
        # and a product with one k-term dropped is outside it
        op = Am.conj().T if herm else Am
        bad = acc - V[:, :1] * op[None, :, 0]
        err = R.err_against(bad, h, l)
        assert (err > R.gemm_tol(Am, V, C=bad, herm=herm)).any()


def test_g_reference_and_gamma_m():
    rng = np.random.default_rng(5)
    A = R.codebook("synth", 20, 12)
    K = A @ A.conj().T
    T = R.rand_vectors(rng, 4, 20, spread=0.0)
    gs, kappa, Binv = R.g_reference(K, T)
    B = np.eye(20) + K
    assert np.allclose((B @ np.asarray(gs, np.complex128).T).T, T, rtol=1e-13, atol=1e-13)
    assert kappa >= 1.0
    Ta = R.norm_attaining(Binv, 3)
    ga, _, _ = R.g_reference(K, Ta)
    assert abs(R.ninf(np.asarray(ga[0], np.complex128)) - R.ninf(Binv)) <= 1e-12 * R.ninf(Binv)
    assert R.gamma_m(20) < 1e-13
