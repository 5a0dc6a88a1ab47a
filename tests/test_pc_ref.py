"""CPU self-test of tests/pc_ref.py: the image encoder against the layout formulas, I + K, the Schur recursion's
measured constant, and the wrong-kernel models, every one of which must fail the comparisons the GPU suite makes, on
the inputs the GPU suite uses."""
import math

import numpy as np
import pytest

import linop_ref as LR
import pc_ref as PR

SMALL = [(1, 1), (17, 15), (33, 17), (48, 100), (49, 129), (121, 40)]


# ---------------------------------------------------------------- images
def _encode_slow(k):
    """The layout comments of ace_private.hip, dword by dword."""
    m, n = k.shape
    d = PR.dims(m, n)
    code = lambda i, q: int(k[i, q]) if (0 <= i < m and 0 <= q < n) else 0
    cH = np.full(d["nH"], 0xFFFFFFFF, np.uint64)
    for rb in range(d["nb32"]):
        kg, j = (2 * rb) >> 3, ((2 * rb) & 7) >> 1
        for ct in range(d["nct"]):
            for o in range(16):
                for h in range(2):
                    w = 0
                    for p in range(2):
                        for u in range(8):
                            w |= code(32 * rb + 16 * p + 8 * h + u, 16 * ct + o) << PR.code_shift(p, u)
                    cH[(((ct * d["nkgH"] + kg) * 16 + o) * 2 + h) * 4 + j] = w
    cA = np.zeros(d["nA"], np.uint64)
    for ct in range(d["mt"]):
        for kg in range(d["nkgA"]):
            for o in range(16):
                for h in range(2):
                    for j in range(4):
                        w = 0
                        for p in range(2):
                            for u in range(8):
                                w |= code(16 * ct + o, 16 * (8 * kg + 2 * j + p) + 8 * h + u) << PR.code_shift(p, u)
                        cA[(((ct * d["nkgA"] + kg) * 16 + o) * 2 + h) * 4 + j] = w
    cR = np.zeros(d["nR"], np.uint64)
    for i in range(m):
        for wd in range(d["nct"]):
            w = 0
            for u in range(16):
                w |= code(i, 16 * wd + u) << (2 * u)
            cR[i * d["nct"] + wd] = w
    return dict(cH=cH.astype(np.uint32), cA=cA.astype(np.uint32), cR=cR.astype(np.uint32))


@pytest.mark.parametrize("m,n", [(1, 1), (17, 15), (33, 17), (49, 129), (100, 40)])
def test_encoder_is_the_layout_and_decodes_back(m, n):
    k = PR.codes(3, m, n)
    enc, slow = PR.encode(k), _encode_slow(k)
    for nm in ("cH", "cA", "cR"):
        assert np.array_equal(enc[nm], slow[nm]), nm
    assert PR.compare_images(slow, k) == []
    dec = PR.decode(enc, m, n)
    for nm in ("cA", "cR"):
        assert np.array_equal(dec[nm], k), nm
    # cH: the rows of the defined K-steps (all of them: 2 nb32 >= mt)
    assert np.array_equal(dec["cH"], k)
    # the undefined dwords are exactly the K-step pairs past nb32 of the last group
    d = PR.dims(m, n)
    assert enc["maskH"].sum() == d["nct"] * 32 * d["nb32"] and (enc["cH"][~enc["maskH"]] == 0xFFFFFFFF).all()


def test_the_codes_of_a_matrix():
    k = PR.codes(5, 7, 9)
    for c in (1.0, 1 / 3.0, 16 / math.sqrt(9)):
        c2, k2 = PR.codes_of(PR.phase_code(k, c))
        assert c2 == c and np.array_equal(k2, k)
    A = PR.phase_code(k, 0.5)
    for bad in (0.5 + 0.5j, 0.25, np.nan, 0.0):
        B = A.copy()
        B[6, 8] = bad
        assert PR.codes_of(B) is None


@pytest.mark.parametrize("model", PR.IMAGE_MODELS)
@pytest.mark.parametrize("m,n", [(33, 17), (49, 129), (17, 100)])
def test_wrong_images_fail(model, m, n):
    k = PR.codes(3, m, n)
    assert PR.compare_images(PR.encode(k, model), k) != []


# ---------------------------------------------------------------- I + K
@pytest.mark.parametrize("m,n", SMALL)
def test_kmat_is_the_product(m, n):
    k = PR.codes(9, m, n, twin=True)
    for c in (1 / math.sqrt(n), 16 / math.sqrt(n), 0.25):
        A = PR.phase_code(k, c)
        a, b = PR.kmat_candidates(k, c)
        K = A @ A.conj().T
        assert np.abs(a[:m, :m] - np.eye(m) - K).max() <= 4 * n * c * c * LR.U * 4
        assert np.array_equal(a[m:, m:], np.eye(a.shape[0] - m)) and not a[:m, m:].any() and not a[m:, :m].any()
        assert PR.kmat_matches(a, k, c) and PR.kmat_matches(b, k, c)
        kr, ki = LR.kint(A)
        assert np.array_equal(kr, PR.kmat_counts(k)[0]) and np.array_equal(ki, PR.kmat_counts(k)[1])
        if m > 1:
            assert a[0, 1] == c * c * n   # the identical rows


@pytest.mark.parametrize("model", PR.KMAT_MODELS)
def test_wrong_kmat_fails(model):
    k = PR.codes(9, 33, 17, twin=True)
    for c in (1 / math.sqrt(17), 0.25):
        assert not PR.kmat_matches(PR.kmat_candidates(k, c, model)[0], k, c)


# ---------------------------------------------------------------- inverses
@pytest.fixture(scope="module")
def schur_ratios():
    out = {}
    for s in PR.INV_SIZES:
        for name, H, _ in PR.inv_inputs(s):
            T, g, kappa = PR.inv_vectors(H)
            out[(s, name)] = (PR.inv_ratio(PR.schur_inverse(H), T, g, kappa), kappa)
    return out


def test_schur_recursion_constant_is_the_recorded_one(schur_ratios):
    worst = max(r for r, _ in schur_ratios.values())
    print("schur_inverse worst err / (u kappa ||g*||):", worst, {k: round(v[0], 4) for k, v in schur_ratios.items()})
    assert PR.SCHUR_CPU / 1.5 <= worst <= 1.5 * PR.SCHUR_CPU
    assert max(r for (s, nm), (r, _) in schur_ratios.items() if not nm.startswith("int-low")) <= 0.5


def test_schur_recursion_inverts_and_the_inputs_are_what_they_claim():
    for s in (32, 96, 160):
        for name, H, m in PR.inv_inputs(s):
            assert np.array_equal(H, H.conj().T) and np.linalg.eigvalsh(H).min() >= 1.0 - 1e-9
            G = PR.schur_inverse(H)
            assert np.abs(G @ H - np.eye(s)).max() <= 1e-10
            if m < s:
                assert np.array_equal(H[m:, m:], np.eye(s - m)) and np.array_equal(G[m:, m:], np.eye(s - m))
            if name.startswith("int"):
                assert np.array_equal(H, np.rint(H.real) + 1j * np.rint(H.imag))


def test_a_wrong_inverse_exceeds_the_bounds():
    """One off-diagonal block with the wrong sign (the -T of the recursion) is far beyond both bounds."""
    s = 96
    name, H, _ = PR.inv_inputs(s)[0]
    T, g, kappa = PR.inv_vectors(H)
    G = PR.schur_inverse(H)
    G[:32, 32:] = -G[:32, 32:]
    r = PR.inv_ratio(G, T, g, kappa)
    assert r > PR.SCHUR_MULT * PR.SCHUR_CPU and r * LR.U > LR.gamma_gj(s)


# ---------------------------------------------------------------- tiles
def test_tiles_round_trip_and_the_effective_matrix():
    rng = np.random.default_rng(0)
    for m in (1, 17, 48, 49, 121):
        R = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
        H = R + R.conj().T
        Gt = PR.tiles_of(H, m)
        assert np.array_equal(PR.g_effective(Gt, m), H)
        # a matrix that is not Hermitian: the upper tiles come from the lower ones, diagonal tiles as stored
        Ge = PR.g_effective(PR.tiles_of(R, m), m)
        ti = np.arange(m) // 16
        low, dia = ti[:, None] > ti[None, :], ti[:, None] == ti[None, :]
        assert np.array_equal(Ge[low], R[low]) and np.array_equal(Ge[dia], R[dia])
        assert np.array_equal(Ge.T[low], R.conj()[low])


# ---------------------------------------------------------------- the digit product
def test_digit_product_is_the_digit_model():
    rng = np.random.default_rng(1)
    k = PR.codes(2, 17, 40)
    EA, EAH = PR.expansions(k)
    for E, cols in ((EA, 80), (EAH, 34)):
        V = LR.edge_vectors(rng, 4, cols // 2).view(np.float64)
        e = LR.kernel_exp(np.max(np.abs(V), axis=1))
        ref = LR.digit_model(E, 0.3, V, e)
        for j in range(4):
            assert np.array_equal(PR.digit_product(E, 0.3, V[j], e[j]), ref[j])


# ---------------------------------------------------------------- one launch
CASES = [dict(m=33, n=17, avok=1), dict(m=33, n=17, avok=0, nzero=0), dict(m=48, n=100, avok=0, nzero=1),
         dict(m=17, n=129, avok=1, own_g=False, yn_id=2, optysrc=2, opt_obj=0.0),
         dict(m=65, n=40, avok=1, yn_id=1, optysrc=2, opt_obj=math.inf)]


def _inputs(case, seed=21):
    kw = {k: v for k, v in case.items() if k not in ("m", "n")}
    inp = PR.step_inputs(case["m"], case["n"], 3, seed, **kw)
    inp["Gt"] = PR.cpu_gt(inp)
    return inp


@pytest.fixture(scope="module")
def launches():
    out = []
    for case in CASES:
        inp = _inputs(case)
        out.append((case, inp, [PR.step_reference(inp, b) for b in range(3)]))
    return out


def test_the_plain_f64_model_passes_every_comparison(launches):
    for case, inp, refs in launches:
        fails, worst = PR.compare_step(PR.model_result(inp), inp, refs=refs)
        assert fails == [], (case, fails)
        assert 0 < max(worst.values()) <= 1.0 and set(worst) == {"AX", "M", "Yn", "W"} | set(PR.SUMS)


def _applicable(model, case):
    if model == "tile_row_dropped":
        return case["m"] <= 48
    if model in ("N_despite_nzero",):
        return not case["avok"] and case.get("nzero")
    if model == "AX_despite_cold":
        return not case["avok"]
    if model == "optysrc_kept":
        return case.get("yn_id") and case.get("optysrc") == case.get("yn_id") and case.get("opt_obj") == 0.0
    if model == "no_zero_guard":
        return False   # (its own inputs below)
    return True


@pytest.mark.parametrize("model", [m for m in PR.MODELS if m != "no_zero_guard"])
def test_every_wrong_kernel_model_fails(launches, model):
    hit = 0
    for case, inp, refs in launches:
        if not _applicable(model, case):
            continue
        hit += 1
        if model == "N_despite_nzero":   # (with a finite stored N as well: not only through the NaN poison)
            inp = dict(inp, N=0.1 * PR.step_inputs(case["m"], case["n"], 3, 5)["Z"])
            refs = None
        fails, _ = PR.compare_step(PR.model_result(inp, model), inp, refs=refs)
        assert fails, (model, case)
    assert hit, model


def zero_guard_inputs(m, n, nb, seed):
    """G = I, AX = 0, M = 0: cc = Yo - Yo = 0 exactly in every entry."""
    inp = PR.step_inputs(m, n, nb, seed, avok=1, own_g=False)
    inp["G"] = np.stack([np.eye(m, dtype=np.complex128)] * nb)
    inp["AX"], inp["M"] = np.zeros((nb, m), np.complex128), np.zeros((nb, m), np.complex128)
    return inp


def test_the_zero_guard_and_its_absence():
    inp = zero_guard_inputs(33, 17, 3, 4)
    inp["Gt"] = PR.cpu_gt(inp)
    refs = [PR.step_reference(inp, b) for b in range(3)]
    assert all(r["zero_guard"].all() for r in refs)
    got = PR.model_result(inp)
    mu = inp["state"][:, PR.SI["mu"]][:, None]
    assert np.array_equal(got["Yn"], ((inp["B"] + mu) / (1 + mu)).astype(np.complex128))
    assert PR.compare_step(got, inp, refs=refs)[0] == []
    assert PR.compare_step(PR.model_result(inp, "no_zero_guard"), inp, refs=refs)[0]


def test_done_realisations_and_the_opt_y_bookkeeping():
    inp = _inputs(dict(m=33, n=17, avok=1, yn_id=1, optysrc=1, opt_obj=math.inf, done=(1,)))
    got = PR.model_result(inp)
    assert PR.compare_step(got, inp)[0] == []
    assert np.array_equal(got["optY"][0], inp["Yn"][0]) and got["flags"][0, PR.FI["optysrc"]] == 1
    assert np.array_equal(got["optY"][1], inp["optY"][1]) and (got["W"][1].view(np.float64) == PR.SENTINEL).all()
    # a done realisation that was stepped all the same, and a deferred copy that did not happen, are caught
    bad = PR.model_result(dict(inp, flags=inp["flags"] * np.array([0, 1, 1, 1], np.int32)))
    bad["flags"] = got["flags"]
    assert any("done" in f for f in PR.compare_step(bad, inp)[0])
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
    bad["optY"][0] = inp["optY"][0]
    assert any("optY" in f for f in PR.compare_step(bad, inp)[0])
    # an array the kernel must not write
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
    bad["Z"][2, 3] *= 1 + 2.0 ** -52
    assert any("Z was written" in f for f in PR.compare_step(bad, inp)[0])


def test_integer_inputs_are_exact():
    inp, want = PR.int_step_inputs(49, 17, 3, 6)
    assert np.array_equal(want, np.rint(want.real) + 1j * np.rint(want.imag)) and np.abs(want).max() < 2.0 ** 52
    ti = np.arange(49) // 16
    up = ti[:, None] < ti[None, :]
    assert np.isnan(inp["G"][0][up]).all() and np.isfinite(inp["G"][0][~up]).all()
    inp["Gt"] = np.stack([PR.tiles_of(inp["G"][b], 49) for b in range(3)])
    assert np.isfinite(inp["Gt"]).all()
    got = PR.model_result(inp)
    assert np.array_equal(got["AX"], want)
    for model in ("G_unconjugated", "diag_twice"):
        assert not np.array_equal(PR.model_result(inp, model)["AX"], want)
