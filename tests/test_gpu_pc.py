"""The private code-image kernels (csrc/ace_private.hip) one launch at a time through ace_pc_host, against the
references and error scales of tests/pc_ref.py (self-tested on the CPU by tests/test_pc_ref.py).

PAIRS covers, by (m, n): mt = ceil(m/16) odd against nb32 = ceil(m/32) (1, 15, 16, 33, 65, 225: mp != mp32), waves
that own no tile row (m <= 48), one against two K-step groups of the A^H image (m <= 128 / above) and of the A image
(n <= 128 / above), every n tail (n not a multiple of 16: the kc < n, k < np and col < 2n guards; n = 1), the
never-written dwords of the A^H image (4 kg + j >= nb32: every m with mt < 8 or 8 < mt < 16) and the LDS ceiling of
pc_supported (256, 2048).  Every test asserts the guards of every buffer and of the control blocks.

End to end the n tails come through a solve with an even tx whose tx * rx is no multiple of 16: the solve accepts
them on this path, and tests/test_gpu_private.py::test_private_phase_code_matches_oracle has tx = 6 (n = 36) and
tx = 10 (n = 100).
"""
import math

import numpy as np
import pytest

import linop_ref as LR
import pc_ref as PR

pytestmark = pytest.mark.gpu

PAIRS = [(1, 1), (15, 15), (16, 16), (17, 17), (31, 127), (32, 128), (33, 17), (48, 100), (49, 129), (65, 256),
         (96, 16), (121, 127), (160, 100), (225, 1000), (256, 129), (256, 256), (17, 1000), (32, 1), (1, 129),
         (121, 15)]
CEILING = (256, 2048)
NB = 3
WORST = {}   # worst err / tol per operation and output, printed by the last test


def _note(op, name, r):
    WORST[(op, name)] = max(WORST.get((op, name), 0.0), float(r))


def _host(op, **kw):
    from ace_amd import pcode
    res = pcode.pc_host(op, **kw)
    assert res.guard_ok, "control-block guard"
    assert res.guards_hold(), [k for k in res.guards if not res.guards_hold([k])]
    return res


def _codebooks(m, n, nb=NB, seed=3):
    inp = PR.step_inputs(m, n, nb, seed)
    return inp["k"], inp["c"], inp["A"]


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("m,n", PAIRS + [CEILING])
def test_pack_images_bit_for_bit(gpu, m, n):
    k, c, A = _codebooks(m, n)
    res = _host("pack", batch=NB, m=m, n=n, A=A)
    assert res.flag == 0 and np.array_equal(res.cb, c)
    for b in range(NB):
        assert PR.compare_images({nm: res.vec[nm][b] for nm in ("cH", "cA", "cR")}, k[b]) == [], b
    # the buffers pack does not write
    for nm in ("Gw", "Gt", "P0", "W", "AX", "Yn"):
        assert (res.vec[nm].view(np.float64) == res.sentinel).all(), nm


@pytest.mark.parametrize("bad", [0.5 + 0.5j, 0.25, float("nan"), 0.0])
@pytest.mark.parametrize("m,n", [(33, 17), (160, 100)])
def test_pack_flags_what_is_no_phase_code(gpu, m, n, bad):
    k, _, _ = _codebooks(m, n)
    A = np.stack([PR.phase_code(k[b], 0.5) for b in range(NB)])
    A[NB - 1, m - 1, n - 1] = bad
    assert PR.codes_of(A[NB - 1]) is None
    assert _host("pack", batch=NB, m=m, n=n, A=A).flag == 1


# ---------------------------------------------------------------- I + K
@pytest.mark.parametrize("m,n", PAIRS + [CEILING])
def test_kmat_is_one_plus_k_exactly(gpu, m, n):
    """c = 1/sqrt(n), 16/sqrt(n) (two identical rows), 1/4 in realisations 0, 1, 2."""
    k, c, A = _codebooks(m, n)
    res = _host("kmat", batch=NB, m=m, n=n, A=A)
    mp32 = PR.dims(m, n)["mp32"]
    for b in range(NB):
        Gw = res.Gw[b]
        assert np.array_equal(Gw[m:, m:], np.eye(mp32 - m)) and not Gw[:m, m:].any() and not Gw[m:, :m].any(), b
        assert PR.kmat_matches(Gw, k[b], c[b]), b
    a, b2 = PR.kmat_candidates(k[2], 0.25)
    assert np.array_equal(a, b2) and np.array_equal(res.Gw[2], a)   # c a power of two: one candidate, bit for bit
    if m > 1:
        assert res.Gw[1][0, 1] == c[1] * c[1] * n and res.Gw[1][1, 0] == c[1] * c[1] * n


# ---------------------------------------------------------------- the inverse launcher
@pytest.mark.parametrize("form", ["schur", "gj"])
@pytest.mark.parametrize("mp32", PR.INV_SIZES)
def test_inverse_of_caller_matrices(gpu, mp32, form):
    """|| g - g* ||_inf <= gamma kappa_inf || g* ||_inf on norm-attaining and random T; gamma = gamma_gj(mp32) for the
    Gauss-Jordan, SCHUR_MULT times the numpy recursion's measured constant for the Schur recursion."""
    cases = PR.inv_inputs(mp32)
    res = _host("inv", batch=len(cases), m=mp32, form=form, Gin=np.stack([H for _, H, _ in cases]))
    bound = LR.gamma_gj(mp32) / LR.U if form == "gj" else PR.SCHUR_MULT * PR.SCHUR_CPU
    for b, (name, H, m) in enumerate(cases):
        T, g, kappa = PR.inv_vectors(H)
        r = PR.inv_ratio(res.Gw[b], T, g, kappa)
        print(f"inv {form} mp32={mp32} {name}: err / (u kappa ||g*||) = {r:.4g} (bound {bound:.4g})")
        _note("inv-" + form, "ratio to u kappa ||g*||", r)
        _note("inv-" + form, "err/tol", r / bound)
        assert r <= bound, (name, r, bound)
        if m < mp32:   # identity rows and columns outside m stay exactly identity
            G = res.Gw[b]
            assert np.array_equal(G[m:, m:], np.eye(mp32 - m)) and not G[:m, m:].any() and not G[m:, :m].any()


# ---------------------------------------------------------------- tiles
@pytest.mark.parametrize("m", [1, 17, 33, 48, 121, 225, 256])
def test_tiles_are_a_rearrangement(gpu, m):
    mp32 = PR.dims(m, 16)["mp32"]
    idx = np.arange(NB * mp32 * mp32, dtype=np.float64).reshape(NB, mp32, mp32)
    Gin = (idx + 1) - 1j * (idx + 0.5)   # distinct per entry, no symmetry
    res = _host("tiles", batch=NB, m=m, Gin=Gin)
    for b in range(NB):
        assert PR.same_bits(res.Gt[b], PR.tiles_of(Gin[b], m)), b


# ---------------------------------------------------------------- P0 = A X0
@pytest.mark.parametrize("m,n", PAIRS + [CEILING])
def test_apply_a_against_the_exact_product(gpu, m, n):
    k, c, A = _codebooks(m, n, nb=4)
    rng = np.random.default_rng([m, n, 5])
    Xi = LR.int_vectors(rng, 4, n)
    res = _host("apply_a", batch=4, m=m, n=n, A=A, X0=Xi)
    for b in range(4):
        hi, lo = LR.exact_cmatvec(A[b], Xi[b][None])
        assert np.array_equal(res.P0[b].view(np.float64), hi[0]), b   # integer data: the correctly rounded product
    for X in (LR.edge_vectors(rng, 4, n), LR.rand_vectors(rng, 4, n)):
        res = _host("apply_a", batch=4, m=m, n=n, A=A, X0=X)
        for b in range(4):
            hi, lo = LR.exact_cmatvec(A[b], X[b][None])
            e = LR.kernel_exp(LR.maxabs_rows(X[b][None]))
            tol = LR.i8_tol(PR.expansions(k[b])[0], c[b], e, hi)
            err = LR.err_against(res.P0[b][None], hi, lo)
            _note("apply_a", "P0", np.max(err / tol))
            assert (err <= tol).all(), (b, np.max(err / tol))


# ---------------------------------------------------------------- one pgk launch
def _step(inp, m, n):
    """One launch; returns (res, got, inp with the kernel's own Gt and the packed c)."""
    nb = len(inp["k"])
    res = _host("step", batch=nb, m=m, n=n, yn_id=inp["yn_id"], A=inp["A"], G=inp["G"], B=inp["B"], Yo=inp["Yo"],
                M=inp["M"], AX=inp["AX"], Yn=inp["Yn"], optY=inp["optY"], Z=inp["Z"], N=inp["N"], state=inp["state"],
                flags=inp["flags"])
    assert res.flag == 0 and np.array_equal(res.cb, inp["c"])
    got = dict(res.vec, state=res.state, flags=res.flags)
    return res, got, dict(inp, Gt=res.Gt)


def _check(inp, m, n, refs=None):
    res, got, full = _step(inp, m, n)
    fails, worst = PR.compare_step(got, full, sentinel=res.sentinel, refs=refs)
    for nm, r in worst.items():
        _note("step", nm, r)
    assert fails == [], fails
    return res, got, full


@pytest.mark.parametrize("m,n", PAIRS)
def test_step_integer_data_is_exact(gpu, m, n):
    """T = Yo - AX and g = G T are exact on integer data: AX' = Yo - g bit for bit, with NaN in the strictly upper
    tiles of the dense G, which are never read."""
    inp, want = PR.int_step_inputs(m, n, NB, 8)
    res, got, _ = _step(inp, m, n)
    assert np.isfinite(got["AX"]).all() and np.array_equal(got["AX"], want)
    assert np.isfinite(got["W"]).all() and np.isfinite(res.state[:, 3:]).all()


@pytest.mark.parametrize("m,n", PAIRS + [CEILING])
def test_step_floating_data(gpu, m, n):
    """Every output through compare_step: the warm branch on the setup's own G, the cold A V branch with N and a
    caller's G, and the cold branch under nzero (the stored N is NaN) on the setup's own G."""
    _check(PR.step_inputs(m, n, NB, 21, avok=1, yn_id=2, optysrc=2), m, n)
    _check(PR.step_inputs(m, n, NB, 22, avok=0, nzero=0, own_g=False, yn_id=1, opt_obj=0.0), m, n)
    inp = PR.step_inputs(m, n, NB, 23, avok=0, nzero=1)
    assert np.isnan(inp["N"]).all()
    _check(inp, m, n)


@pytest.mark.parametrize("m,n", [(33, 17), (160, 100)])
def test_step_zero_guard(gpu, m, n):
    """G = I, AX = 0, M = 0: cc = 0 exactly, and Yn = (B + mu) / (1 + mu)."""
    inp = PR.step_inputs(m, n, NB, 4, avok=1, own_g=False)
    inp["G"] = np.stack([np.eye(m, dtype=np.complex128)] * NB)
    inp["AX"], inp["M"] = np.zeros((NB, m), np.complex128), np.zeros((NB, m), np.complex128)
    res, got, full = _check(inp, m, n)
    mu = inp["state"][:, PR.SI["mu"]][:, None]
    assert np.array_equal(got["Yn"], ((inp["B"] + mu) / (1 + mu)).astype(np.complex128))
    assert not got["AX"].any()


def test_step_opt_y_decision_and_bookkeeping(gpu):
    m, n, nb = 33, 17, 4
    base = PR.step_inputs(m, n, nb, 31, avok=1)
    res, _, full = _step(base, m, n)
    refs = [PR.step_reference(full, b) for b in range(nb)]
    obj = sorted(math.sqrt(float(r["obj2"][0])) for r in refs)
    assert obj[2] - obj[1] > 1e-3 * obj[2]
    for opt in (math.inf, 0.0, 0.5 * (obj[1] + obj[2])):
        margins = [PR.decision(r, opt)[1] for r in refs]
        assert min(margins) > 1e6, margins   # far from a tie on the reference
        nimp = sum(PR.decision(r, opt)[0] for r in refs)
        assert nimp == {math.inf: nb, 0.0: 0}.get(opt, 2)
        for yn_id, srcs in ((0, (0,)), (1, (0, 1, 2)), (2, (0, 2, 1))):
            for src in srcs:
                inp = dict(base, yn_id=yn_id, state=base["state"].copy(), flags=base["flags"].copy())
                inp["state"][:, PR.SI["opt_obj"]] = opt
                inp["flags"][:, PR.FI["optysrc"]] = src
                _, got, _ = _check(inp, m, n, refs=refs)
                for b in range(nb):
                    imp = PR.decision(refs[b], opt)[0]
                    if yn_id == 0:
                        assert PR.same_bits(got["optY"][b], got["Yn"][b] if imp else base["optY"][b])
                    else:
                        assert PR.same_bits(got["optY"][b], base["Yn"][b] if src == yn_id else base["optY"][b])
                        assert got["flags"][b, PR.FI["optysrc"]] == (yn_id if imp else (0 if src == yn_id else src))


def test_step_done_realisations_are_left_alone(gpu):
    m, n, nb = 49, 129, 5
    inp = PR.step_inputs(m, n, nb, 41, avok=0, yn_id=1, optysrc=1, done=(0, 3))
    res, got, _ = _check(inp, m, n)
    for b in (0, 3):
        for nm in ("AX", "M", "Yn", "optY"):
            assert PR.same_bits(got[nm][b], inp[nm][b]), (b, nm)
        assert (got["W"][b].view(np.float64) == res.sentinel).all()
        assert PR.same_bits(got["state"][b], inp["state"][b]) and np.array_equal(got["flags"][b], inp["flags"][b])
    # and with no buffer supplied the untouched rows still hold the sentinel
    bare = dict(inp, AX=None, Yn=None, optY=None, flags=inp["flags"].copy())
    bare["flags"][:, PR.FI["optysrc"]] = 0
    _, got2, _ = _step(bare, m, n)
    for b in (0, 3):
        for nm in ("AX", "Yn", "optY"):
            assert (got2[nm][b].view(np.float64) == res.sentinel).all(), (b, nm)


@pytest.mark.parametrize("m,n", [(33, 17), (225, 1000)])
def test_step_placement_in_the_batch(gpu, m, n):
    """A realisation's outputs are bit identical alone, first and last in a batch of 5."""
    inp = PR.step_inputs(m, n, 5, 51, avok=0, yn_id=2)

    def pick(order):
        sub = {k_: (np.ascontiguousarray(v[order]) if isinstance(v, np.ndarray) else v) for k_, v in inp.items()}
        _, got, _ = _step(sub, m, n)
        return got
    alone, first, last = pick([2]), pick([2, 0, 1, 3, 4]), pick([0, 1, 3, 4, 2])
    for nm in ("AX", "M", "Yn", "W", "optY", "state", "flags"):
        assert PR.same_bits(alone[nm][0], first[nm][0]) and PR.same_bits(alone[nm][0], last[nm][4]), nm


@pytest.mark.parametrize("m,n", [(48, 100), (121, 127)])
def test_step_two_chained_launches(gpu, m, n):
    """The ping-pong pair swapped as the solve swaps it (yn_id 2, then 1): each launch against the reference on what
    the launch before handed back, the second one reusing the first one's AX (avok = 1)."""
    from ace_amd import pcode
    inp = PR.step_inputs(m, n, NB, 61, avok=0, yn_id=2, optysrc=0)
    res, got, _ = _check(inp, m, n)
    assert (res.flags[:, PR.FI["optysrc"]] == 2).all()   # opt_obj = inf: the best Y is the one just written
    nxt = res.next()
    nxt["flags"] = nxt["flags"].copy()
    nxt["flags"][:, PR.FI["avok"]] = 1
    nxt["state"] = nxt["state"].copy()
    nxt["state"][:, PR.SI["opt_obj"]] = 0.0   # no improvement in the second launch: the deferred copy must happen
    inp2 = dict(inp, yn_id=1, **nxt)
    assert PR.same_bits(inp2["Yo"], got["Yn"]) and PR.same_bits(inp2["AX"], got["AX"])
    res2, got2, full2 = _check(inp2, m, n)
    # the launch overwrote buffer 1 ... and buffer 2 (now Yo) still holds the best Y: optysrc stays 2, no copy yet
    assert (res2.flags[:, PR.FI["optysrc"]] == 2).all() and PR.same_bits(got2["optY"], inp["optY"])
    # a third launch writes buffer 2: the best Y moves to optY first
    nxt = res2.next()
    inp3 = dict(inp2, yn_id=2, **nxt)
    res3, got3, _ = _check(inp3, m, n)
    assert PR.same_bits(got3["optY"], got["Yn"]) and (res3.flags[:, PR.FI["optysrc"]] == 0).all()
    assert pcode.STATE == PR.STATE and pcode.FLAGS == PR.FLAGS


def test_zz_worst_ratios(gpu):
    """Prints the worst err / tol per operation of this run (the figures quoted in DESIGN.md)."""
    for (op, nm), r in sorted(WORST.items()):
        print(f"worst {op} {nm}: {r:.4g}")
    assert all(r <= 1.0 for (op, nm), r in WORST.items() if nm != "ratio to u kappa ||g*||")
