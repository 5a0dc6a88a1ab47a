"""GPU tests of the batched OMP (ace_omp_solve_*, csrc/ace_omp.hip).

Target: the longdouble reference of tests/omp_ref.py.  idx and count are compared exactly (tests/test_omp_ref.py
asserts, for every realisation, the conditions that make them well defined); coef and resnorm inside the tolerances
derived there from the kernel's least-squares method (modified Gram-Schmidt QR on [D_I y], backward stable):
eps = 8 (d + 2 k + 2) u, ||dc|| <= eps (kappa (||c|| + ||y|| / smax) + kappa^2 ||r|| / smax),
| d||r|| | <= eps (smax ||c|| + ||y|| + kappa ||r||).

A work-group owns 16 realisations, a wave walks the atoms in pairs of 16-atom tiles, the k loop runs in chunks of 16
rows, a group of 32 lanes owns a realisation's d-vector.  The shapes cover: the minimum; d below one chunk and
above (5, 17), N below a tile and not a multiple of one (7, 130, 300, 2401, 1000), more atoms than 8 waves x 32
(300 and up), one full block, a partial one and three (16, 17, 33 realisations), d = 256 = the limit, kmax = d.

Worst err / tol measured on the MI355X over all parity cases: coef 0.032 and resnorm 0.030 at (1, 1, 1, 1); from
(3, 5, 7, 5) on both stay below 0.007 (the bound is a worst case over d + 2 k roundings; DESIGN.md §4f has the table).
"""
import ctypes as C
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import omp_ref as OR  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(s, w, m) for s in OR.SHAPES + [OR.TWO_STAGE] for w in (False, True) for m in ("count", "tol")]
IDS = [("x".join(map(str, s)) if s != OR.TWO_STAGE else s) + ("-colscale" if w else "") + f"-{m}" for s, w, m in CASES]


def _dev(gpu, *arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).to(gpu) for a in arrays]


def _np(res):
    """(idx, coef, count, resnorm, status as uint32, x or None) on the host."""
    x = None if res.x is None else res.x.cpu().numpy()
    return (res.idx.cpu().numpy(), res.coef.cpu().numpy(), res.count.cpu().numpy(), res.resnorm.cpu().numpy(),
            res.status.cpu().numpy().view(np.uint32), x)


def _same(a, b):
    return all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(a, b))


def _check_layout(idx, coef, count, x, N):
    """-1 / 0 past count, distinct indices, x = the scatter of coef."""
    for b in range(idx.shape[0]):
        k = count[b]
        assert (idx[b, k:] == -1).all() and (coef[b, k:] == 0).all()
        assert len(set(idx[b, :k].tolist())) == k and (idx[b, :k] >= 0).all() and (idx[b, :k] < N).all()
        if x is not None:
            want = np.zeros(N, np.complex128)
            want[idx[b, :k]] = coef[b, :k]
            assert np.array_equal(x[b], want)


@pytest.mark.parametrize("shape,scaled,mode", CASES, ids=IDS)
def test_parity_with_the_extended_precision_reference(gpu, shape, scaled, mode):
    from ace_amd import omp_batch
    c = OR.case(shape, scaled)
    tol = 0.0 if mode == "count" else OR.tol_for(c)
    D, Y, w = _dev(gpu, c["D"], c["Y"], c["w"])
    idx, coef, count, rn, st, x = _np(omp_batch(D, Y, c["kmax"], tol, w, want_x=True))
    exp = OR.expected(c, tol)
    assert (st == 0).all()
    assert count.tolist() == [e["count"] for e in exp]
    for b, e in enumerate(exp):
        assert idx[b, :e["count"]].tolist() == e["idx"], b
    _check_layout(idx, coef, count, x, c["D"].shape[1])
    q = OR.ratios(c, tol, idx, coef, count, rn)
    print(f"{shape} colscale={scaled} {mode}: worst err/tol " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q


WRONG = {"no-conjugate": dict(conj=False), "real-part": dict(select="real"), "no-exclusion": dict(exclude=False),
         "correlation-coefficients": dict(coef="corr")}


@pytest.mark.parametrize("name", list(WRONG))
def test_wrong_models_are_rejected(gpu, name):
    """Each wrong numpy model differs from the kernel in idx, or lands outside the tolerance, on every realisation
    of these inputs; the right model (the same code with no switch) agrees on all of them."""
    from ace_amd import omp_batch
    if name == "no-exclusion":
        # In exact arithmetic the residual is orthogonal to the chosen atoms, so exclusion only matters where their
        # rounding-level correlation can win: a dictionary with a duplicated column, and a colscale of 1e40 on the
        # first of the twins.  It is picked first; afterwards 1e40 times its correlation's rounding residue
        # (about (1e-16)^2) beats every honest candidate, so a model without exclusion picks it again and stalls,
        # while its twin (weight 1) stays at rounding level for both.
        rng = np.random.default_rng(11)
        D = OR._cn(rng, 12, 40)
        D /= np.linalg.norm(D, axis=0)
        D[:, 30] = D[:, 4]
        Y = np.stack([(2.0 + b) * D[:, 4] + D[:, 9 + b] + 0.02 * OR._cn(rng, 12) for b in range(4)])
        kmax, w = 3, np.ones(40)
        w[4] = 1e40
    else:
        c = OR.case((33, 17, 130, 8), True)
        D, Y, w, kmax = c["D"], c["Y"], c["w"], c["kmax"]
    Dd, Yd, wd = _dev(gpu, D, Y, w)
    idx, coef, count, rn, st, _ = _np(omp_batch(Dd, Yd, kmax, 0.0, wd))
    d = D.shape[0]
    eps = 8.0 * (d + 2 * kmax + 2) * OR.U
    for b in range(Y.shape[0]):
        good = OR.model(D, Y[b], kmax, 0.0, w)
        k = len(good["idx"])
        sv = np.linalg.svd(D[:, good["idx"]], compute_uv=False)
        kap = sv[0] / sv[-1]
        tolc = 2 * eps * (kap * (np.linalg.norm(good["coef"]) + np.linalg.norm(Y[b]) / sv[0])
                          + kap * kap * float(good["norms"][-1]) / sv[0])   # (2: the f64 model has the same error)
        assert idx[b, :count[b]].tolist() == good["idx"] and np.linalg.norm(coef[b, :k] - good["coef"]) <= tolc
        bad = OR.model(D, Y[b], kmax, 0.0, w, **WRONG[name])
        differs = bad["idx"] != good["idx"] or np.linalg.norm(bad["coef"] - coef[b, :k]) > tolc
        assert differs, (name, b)


def test_ties_go_to_the_smaller_index_and_the_duplicate_is_never_chosen(gpu):
    """Columns 2, 5 and 9 are bit-identical, and the signal sits on them: index 2 wins the tie whatever lane and
    wave met the twins, and the twins are never chosen afterwards (their correlation with the new residual is
    rounding noise: the run continues with other atoms)."""
    from ace_amd import omp_batch
    rng = np.random.default_rng(3)
    N = 70   # (three tile pairs: the twins 2, 5 share a tile, 40 and 69 sit in other waves' tiles)
    D = OR._cn(rng, 20, N)
    for j in (5, 40, 69):
        D[:, j] = D[:, 2]
    Y = np.stack([3.0 * D[:, 2] + 0.5 * D[:, 11 + b] + 0.2 * D[:, 50 + b] + 0.05 * OR._cn(rng, 20) for b in range(5)])
    Dd, Yd = _dev(gpu, D, Y)
    idx, coef, count, rn, st, _ = _np(omp_batch(Dd, Yd, 4, 0.0))
    assert (count == 4).all() and (st == 0).all()
    for b in range(5):
        m = OR.model(D, Y[b], 4)
        assert m["margins"][0] == 0.0 and min(m["margins"][1:]) > 1e-3   # an exact tie first, clear picks after it
        assert idx[b].tolist() == m["idx"] and idx[b, 0] == 2
        assert not set(idx[b].tolist()) & {5, 40, 69}
        assert {11 + b, 50 + b} <= set(idx[b].tolist())
    # the signal exactly on the twins, nothing else: after index 2 the residual is rounding noise, and whatever is
    # picked on it, no twin is ever added (a twin that wins the noise is dependent and stops the run)
    idx, coef, count, rn, st, _ = _np(omp_batch(Dd, _dev(gpu, np.stack([3.0 * D[:, 2]]))[0], 4, 0.0))
    assert idx[0, 0] == 2 and not set(idx[0].tolist()) & {5, 40, 69}


def test_exhaustion_is_sound(gpu):
    """The faithful setting of the two-stage recovery: tol = 1e-12, kmax = d, noisy y, at (4, 46, 625).  The late
    picks are made on rounding noise, so there is no parity: only soundness, with the bounds of tests/omp_ref.py
    from the final support's own singular values."""
    from ace_amd import omp_batch
    rng = np.random.default_rng(8)
    batch, d, N = 4, 46, 625
    D = OR._cn(rng, d, N)
    D /= np.linalg.norm(D, axis=0)
    Y = np.stack([D[:, rng.choice(N, 3, replace=False)] @ OR._cn(rng, 3) + 0.03 * OR._cn(rng, d) for _ in range(batch)])
    Dd, Yd = _dev(gpu, D, Y)
    idx, coef, count, rn, st, x = _np(omp_batch(Dd, Yd, d, 1e-12, want_x=True))
    _check_layout(idx, coef, count, x, N)
    for b in range(batch):
        k = count[b]
        assert 1 <= k <= d
        I = idx[b, :k]
        sv = np.linalg.svd(D[:, I], compute_uv=False)
        kap, smax = sv[0] / sv[-1], sv[0]
        ny, nc = np.linalg.norm(Y[b]), np.linalg.norm(coef[b, :k])
        eps = 8.0 * (d + 2 * k + 2) * OR.U
        r = (Y[b].astype(OR.CLD) - D[:, I].astype(OR.CLD) @ coef[b, :k].astype(OR.CLD))
        true_rn = float(np.sqrt(np.sum(np.abs(r) ** 2)))
        bound = eps * (smax * nc + ny + kap * true_rn)
        print(f"exhaustion b={b}: count {k}, kappa {kap:.1f}, resnorm {rn[b]:.3e}, recomputed {true_rn:.3e}, bound {bound:.3e}")
        assert abs(rn[b] - true_rn) <= bound
        for p in range(1, k + 1):   # no prefix of the support fits y better
            ls = np.linalg.lstsq(D[:, I[:p]], Y[b], rcond=None)[0]
            assert rn[b] <= np.linalg.norm(Y[b] - D[:, I[:p]] @ ls) + bound
        assert k == d or rn[b] <= 1e-12 or st[b] != 0   # stopped for a reason


def test_degenerate_inputs(gpu):
    from ace_amd import omp_batch, ACE_ST_EVAL_DEGENERATE, ACE_ST_OMP_DEPENDENT
    c = OR.case((17, 16, 64, 3), False)
    Yh = np.array(c["Y"][:5])
    Yh[1, 7] = complex(np.nan, 0.0)
    Yh[2, 15] = complex(0.0, np.inf)
    Yh[3] = 0
    D, Y, Yp = _dev(gpu, c["D"], Yh, c["Y"][:5])
    res = omp_batch(D, Y, 3, 0.0, want_x=True)
    idx, coef, count, rn, st, x = _np(res)
    plain = _np(omp_batch(D, Yp, 3, 0.0, want_x=True))
    assert st.tolist() == [0, ACE_ST_EVAL_DEGENERATE, ACE_ST_EVAL_DEGENERATE, 0, 0]
    assert res.degenerate.cpu().numpy().tolist() == [False, True, True, False, False]
    for b in (1, 2, 3):
        assert count[b] == 0 and (idx[b] == -1).all() and (coef[b] == 0).all() and rn[b] == 0 and not x[b].any()
    for b in (0, 4):   # the neighbours are untouched bit for bit
        assert _same([a[b] for a in (idx, coef, count, rn, st, x)], [a[b] for a in plain])
    # ||y|| <= tol: count 0, no flag, resnorm = ||y||
    big = _np(omp_batch(D, Yp, 3, 1e3))
    assert (big[2] == 0).all() and (big[4] == 0).all() and np.allclose(big[3], np.linalg.norm(c["Y"][:5], axis=1), rtol=1e-14)
    # a rank-deficient dictionary: 6 copies of 2 distinct columns, kmax = 4 -> two atoms, then dependence
    rng = np.random.default_rng(2)
    a, bcol = OR._cn(rng, 9), OR._cn(rng, 9)
    Dr = np.stack([a, bcol, a, bcol, a, bcol], axis=1)
    Yr = np.stack([2.0 * a + 0.7 * bcol + 0.3 * OR._cn(rng, 9) for _ in range(3)])
    Dd, Yd = _dev(gpu, Dr, Yr)
    r2 = omp_batch(Dd, Yd, 4, 0.0)
    idx, coef, count, rn, st, _ = _np(r2)
    assert (st == ACE_ST_OMP_DEPENDENT).all() and r2.dependent.cpu().numpy().all() and (count == 2).all()
    assert all(sorted(row[:2].tolist()) == [0, 1] and (row[2:] == -1).all() for row in idx)
    for b in range(3):
        ls = np.linalg.lstsq(Dr[:, idx[b, :2]], Yr[b], rcond=None)[0]
        assert np.allclose(coef[b, :2], ls, rtol=1e-12, atol=0)


def _capi(gpu, D, Y, w, kmax, tol, G=64, want_x=True, ws_short=0):
    """ace_omp_solve_batch on inputs and outputs embedded in NaN- / sentinel-filled buffers: returns the outputs and
    whether every guard word is intact."""
    import torch
    from ace_amd._lib import LIB
    batch, d = Y.shape
    N = D.shape[1]

    def guarded(t, fill):
        flat = torch.view_as_real(t).reshape(-1) if t.is_complex() else t.reshape(-1)
        buf = torch.full((flat.numel() + 2 * G,), fill, dtype=flat.dtype, device=gpu)
        buf[G:G + flat.numel()] = flat
        return buf

    ins = [guarded(t, float("nan")) for t in (D, Y)] + ([guarded(w, float("nan"))] if w is not None else [])
    outs = {"idx": torch.full((batch * kmax + 2 * G,), -77, dtype=torch.int32, device=gpu),
            "coef": torch.full((2 * batch * kmax + 2 * G,), -77.0, dtype=torch.float64, device=gpu),
            "count": torch.full((batch + 2 * G,), -77, dtype=torch.int32, device=gpu),
            "resnorm": torch.full((batch + 2 * G,), -77.0, dtype=torch.float64, device=gpu),
            "status": torch.full((batch + 2 * G,), -77, dtype=torch.int32, device=gpu),
            "x": torch.full((2 * batch * N + 2 * G,), -77.0, dtype=torch.float64, device=gpu)}
    nb = int(LIB.ace_omp_workspace_size(batch, d, N, kmax))
    ws = torch.full((nb + 2 * G * 8,), 0x5A, dtype=torch.uint8, device=gpu)
    p = lambda t: t.data_ptr() + G * t.element_size()  # noqa: E731
    rc = LIB.ace_omp_solve_batch(batch, d, N, kmax, tol, p(ins[0]), p(ins[2]) if w is not None else None, p(ins[1]),
                                 p(outs["idx"]), p(outs["coef"]), p(outs["count"]), p(outs["resnorm"]), p(outs["status"]),
                                 p(outs["x"]) if want_x else None, ws.data_ptr() + G * 8, nb - ws_short,
                                 torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    intact = all(bool((t[:G] == -77).all()) and bool((t[-G:] == -77).all()) for t in outs.values())
    intact = intact and bool((ws[:G * 8] == 0x5A).all()) and bool((ws[-G * 8:] == 0x5A).all())
    if not want_x:
        intact = intact and bool((outs["x"] == -77).all())
    body = {k: t[G:-G].cpu().numpy() for k, t in outs.items()}
    return rc, intact, body


def test_guard_regions(gpu):
    """Inputs inside NaN-filled buffers and outputs inside sentinel-filled ones at the odd shape (33, 17, 130, 8):
    the same bits as from plain tensors (a read past an input's end would bring a NaN in), and nothing outside the
    outputs or the workspace is written."""
    from ace_amd import omp_batch
    c = OR.case((33, 17, 130, 8), True)
    D, Y, w = _dev(gpu, c["D"], c["Y"], c["w"])
    want = _np(omp_batch(D, Y, 8, 0.0, w, want_x=True))
    rc, intact, body = _capi(gpu, D, Y, w, 8, 0.0)
    assert rc == 0 and intact
    assert np.array_equal(body["idx"].reshape(33, 8), want[0])
    assert np.array_equal(body["coef"].view(np.complex128).reshape(33, 8), want[1])
    assert np.array_equal(body["count"], want[2]) and np.array_equal(body["resnorm"], want[3])
    assert np.array_equal(body["status"].view(np.uint32), want[4])
    assert np.array_equal(body["x"].view(np.complex128).reshape(33, 130), want[5])
    rc, intact, body = _capi(gpu, D, Y, None, 8, OR.tol_for(c), want_x=False)
    assert rc == 0 and intact


def test_bit_identity_alone_at_an_offset_without_x_on_a_stream_and_on_the_host(gpu):
    """A realisation's outputs are a function of (y_b, D, colscale, d, N, kmax, tol) alone."""
    import torch
    from ace_amd import omp_batch, omp_host
    c = OR.case((33, 17, 130, 8), True)
    tol = OR.tol_for(c)
    D, Y, w = _dev(gpu, c["D"], c["Y"], c["w"])
    full = _np(omp_batch(D, Y, 8, tol, w, want_x=True))
    assert len(set(full[2].tolist())) > 1   # (the realisations of a block stop at different steps)
    for b in range(33):   # each realisation alone: batch 1, column 0 of its block
        one = _np(omp_batch(D, Y[b:b + 1], 8, tol, w, want_x=True))
        assert _same(one, [a[b:b + 1] for a in full]), b
    sub = _np(omp_batch(D, Y[20:], 8, tol, w, want_x=True))
    assert _same(sub, [a[20:] for a in full])
    bare = omp_batch(D, Y, 8, tol, w)
    assert bare.x is None and _same(_np(bare)[:5], full[:5])
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        on_s = omp_batch(D, Y, 8, tol, w, want_x=True)
    s.synchronize()
    explicit = omp_batch(D, Y, 8, tol, w, want_x=True, stream=s)
    s.synchronize()
    assert _same(_np(on_s), full) and _same(_np(explicit), full)
    h = omp_host(c["D"], c["Y"], 8, tol, c["w"], want_x=True)
    assert _same((h.idx, h.coef, h.count, h.resnorm, h.status, h.x), full)


def test_argument_errors_come_before_any_hip_call(gpu):
    """Bad sizes, NULL outputs and a short workspace: the error code, its text, and the sentinel-filled outputs
    untouched."""
    from ace_amd._lib import LIB, ACE_ERR_ARG, ACE_ERR_UNSUPPORTED, ACE_ERR_WORKSPACE
    c = OR.case((3, 5, 7, 5), False)
    D, Y = _dev(gpu, c["D"], c["Y"])
    rc, intact, body = _capi(gpu, D, Y, None, 5, 0.0, ws_short=1)
    assert rc == ACE_ERR_WORKSPACE and b"workspace" in LIB.ace_last_error()
    assert intact and all((v == -77).all() for v in body.values())
    one = C.c_void_p(16)   # never dereferenced: the checks come first
    args = lambda **k: [k.get("batch", 3), k.get("d", 5), k.get("N", 7), k.get("kmax", 5), k.get("tol", 0.0), one, None,  # noqa: E731
                        one, k.get("idx", one), one, one, one, None, None, one, 1 << 30, None]
    assert LIB.ace_omp_solve_batch(*args(d=257, kmax=1)) == ACE_ERR_UNSUPPORTED and b"d 257" in LIB.ace_last_error()
    assert LIB.ace_omp_solve_batch(*args(kmax=6)) == ACE_ERR_ARG and b"kmax" in LIB.ace_last_error()
    assert LIB.ace_omp_solve_batch(*args(N=4)) == ACE_ERR_ARG
    assert LIB.ace_omp_solve_batch(*args(N=16385)) == ACE_ERR_UNSUPPORTED
    assert LIB.ace_omp_solve_batch(*args(idx=None)) == ACE_ERR_ARG and b"NULL idx" in LIB.ace_last_error()
    assert LIB.ace_omp_solve_batch(*args(tol=-1.0)) == ACE_ERR_ARG
    assert LIB.ace_omp_solve_batch(*args(tol=float("nan"))) == ACE_ERR_ARG
    assert LIB.ace_omp_solve_batch(*args(batch=0)) == ACE_ERR_ARG
    assert LIB.ace_omp_workspace_size(3, 257, 7, 5) == 0 and LIB.ace_omp_workspace_size(3, 5, 7, 6) == 0
    assert LIB.ace_omp_workspace_size(3, 5, 7, 5) >= 3 * (25 + 25 + 5) * 16
