"""GPU tests of the beam scan (ace_beam_scan_*: MyBeamSweeping.m's exhaustive sweep and the angular map of
Sparse_Channel_Formulation.m:149 on the device, csrc/ace_scan.hip).

Target: the exact reference of tests/scan_ref.py (products without rounding or in longdouble, modulus, sums and
selection in longdouble) inside the tolerance derived there from the kernel's own accumulation: per entry of y
4 (d0 + d1 + 8) u (sum_ij |W0[q][i]| |x_ij| |F1[p][j]| + |noise|), propagated to P = |y + noise|^2 and to the total.
top_idx, the status word and the values of degenerate realisations are compared exactly; tests/test_scan_ref.py
asserts the gap precondition that makes equal indices well defined.

A work-group owns one realisation and walks the beam pairs in 64 x 64 tiles, so the shapes cover: the minimum;
K-loop tails on both products (d0 = 3, d1 = 5; 17, 31); masked beam tiles (Q = 7, 2, 49, 95, 33, 20, 1) and full
ones (64, 128); several tiles per side (95, 128, 130); K = 1, 3 / 4, 5 / 16 (the three list sizes) and a 1-D scan.

Worst err / tol measured on the MI355X over all parity cases: power 0.022 at (3, 3, 5, 7, 2, 3), top_pow 0.014 and
total 0.013 at (1, 1, 1, 1, 1, 1); from 16 x 16 on power stays below 0.01 and the total below 0.001.
"""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import scan_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(s, k, nz) for s in SR.SHAPES for k in SR.KINDS for nz in (False, True)]
IDS = ["x".join(map(str, s)) + f"-{k}" + ("-noise" if nz else "") for s, k, nz in CASES]


def _dev(gpu, *arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).to(gpu) for a in arrays]   # (copies: the inputs are read-only)


def _np(res):
    """(top_pow, top_idx, status as uint32, total or None, power [batch][Q1*Q0] or None) on the host."""
    tot = None if res.total is None else res.total.cpu().numpy()
    pw = None if res.power is None else res.power.cpu().numpy().reshape(res.power.shape[0], -1)
    return res.top_pow.cpu().numpy(), res.top_idx.cpu().numpy(), res.status.cpu().numpy().view(np.uint32), tot, pw


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("shape,kind,with_noise", CASES, ids=IDS)
def test_parity_with_the_exact_reference(gpu, shape, kind, with_noise):
    from ace_amd import beam_scan_batch, beam_scan_host
    c = SR.case(shape, kind)
    K, ref = c["K"], c["ref_noise" if with_noise else "ref"]
    nz = c["noise"] if with_noise else None
    X, W0, F1, nzd = _dev(gpu, c["X"], c["W0"], c["F1"], nz)
    res = beam_scan_batch(X, W0, F1, K, nzd, want_power=True, want_total=True)
    tp, ti, st, tot, pw = _np(res)
    assert (st == 0).all() and not res.degenerate.any()
    q = SR.ratios(ref, power=pw, top_pow=tp, total=tot)
    print(f"{shape} {kind} noise={with_noise}: worst err/tol " + " ".join(f"{k} {v:.3f}" for k, v in q.items()))
    assert max(q.values()) <= 1.0, q
    assert np.array_equal(ti, ref["top_idx"])
    Q0 = shape[3]
    assert np.array_equal(res.p.cpu().numpy(), ti // Q0) and np.array_equal(res.q.cpu().numpy(), ti % Q0)
    assert np.array_equal(tp, np.take_along_axis(pw, ti.astype(np.int64), axis=1))   # top_pow are entries of the map
    # the host entry runs the same kernel on copies: the same bits
    h = beam_scan_host(c["X"], c["W0"], c["F1"], K, nz, want_power=True, want_total=True)
    assert _same((h.top_pow, h.top_idx, h.status, h.total, h.power.reshape(shape[0], -1)), (tp, ti, st, tot, pw))
    assert np.array_equal(h.p, ti // Q0) and np.array_equal(h.q, ti % Q0)


@pytest.mark.parametrize("all_equal", [False, True], ids=["duplicated-rows", "all-equal"])
def test_exact_ties_go_to_the_smaller_index(gpu, all_equal):
    """Every product is exact in f64: the map equals the reference bit for bit, and tied pairs come out smaller
    index first whatever lane and wave held them."""
    from ace_amd import beam_scan_batch
    c = SR.tie_case(all_equal)
    ref, K = c["ref"], c["K"]
    X, W0, F1, nz = _dev(gpu, c["X"], c["W0"], c["F1"], c["noise"])
    tp, ti, st, tot, pw = _np(beam_scan_batch(X, W0, F1, K, nz, want_power=True, want_total=True))
    assert (st == 0).all()
    assert np.array_equal(pw, ref["power"].astype(np.float64))
    assert np.array_equal(ti, ref["top_idx"]) and np.array_equal(tp, ref["top_pow"].astype(np.float64))
    assert np.array_equal(tot, ref["total"].astype(np.float64))   # (integers below 2^53: every order gives the same sum)
    if all_equal:
        assert ti.tolist() == [list(range(16))] * 4 and (tp == 1.0).all()
    else:
        assert any(len(set(row)) < K for row in tp.tolist())      # (the case does hold ties among its leaders)
    for k in (1, 4, 5):   # the other list sizes: prefixes of the same sequence
        tpk, tik, *_ = _np(beam_scan_batch(X, W0, F1, k, nz))
        assert np.array_equal(tik, ti[:, :k]) and np.array_equal(tpk, tp[:, :k])


def test_bit_identity_alone_at_an_offset_without_outputs_on_a_stream_and_on_the_host(gpu):
    """A realisation's numbers are a function of (x_b, W0, F1, noise_b, the sizes, K) alone."""
    import torch
    from ace_amd import beam_scan_batch, beam_scan_host
    shape = (33, 16, 16, 49, 49, 3)
    rng = np.random.default_rng(5)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)   # noqa: E731
    Xh, Wh, Fh, nh = c(33, 256), c(49, 16), c(49, 16), c(33, 49 * 49)
    X, W0, F1, nz = _dev(gpu, Xh, Wh, Fh, nh)
    K = shape[5]
    full = _np(beam_scan_batch(X, W0, F1, K, nz, want_power=True, want_total=True))
    for b in range(33):   # each realisation alone: batch 1, b = 0
        one = _np(beam_scan_batch(X[b:b + 1], W0, F1, K, nz[b:b + 1], want_power=True, want_total=True))
        assert _same(one, [a[b:b + 1] for a in full]), b
    sub = _np(beam_scan_batch(X[20:], W0, F1, K, nz[20:], want_power=True, want_total=True))
    assert _same(sub, [a[20:] for a in full])
    bare = beam_scan_batch(X, W0, F1, K, nz)
    assert bare.power is None and bare.total is None
    assert _same(_np(bare)[:3], full[:3])
    only_total = _np(beam_scan_batch(X, W0, F1, K, nz, want_total=True))
    assert _same(only_total[:4], full[:4])
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        on_s = beam_scan_batch(X, W0, F1, K, nz, want_power=True, want_total=True)
    explicit = beam_scan_batch(X, W0, F1, K, nz, want_power=True, want_total=True, stream=s)
    s.synchronize()
    assert _same(_np(on_s), full) and _same(_np(explicit), full)
    h = beam_scan_host(Xh, Wh, Fh, K, nh, want_power=True, want_total=True)
    assert _same((h.top_pow, h.top_idx, h.status, h.total, h.power.reshape(33, -1)), full)
    # without noise as well (another argument, not another code path for the product)
    f0 = _np(beam_scan_batch(X, W0, F1, K, want_power=True))
    z0 = _np(beam_scan_batch(X, W0, F1, K, torch.zeros_like(nz), want_power=True))
    assert _same(f0, z0)


def test_degenerate_rows(gpu):
    """A NaN in x or in the realisation's noise row: powers 0, indices -1, total 0 and the flag; the neighbours
    are untouched bit for bit.  An all-zero x is not degenerate: powers 0 and, without noise, indices 0 .. K - 1."""
    from ace_amd import beam_scan_batch
    c = SR.case((17, 16, 16, 64, 64, 4), "random")
    K = 4
    Xh, nh = np.array(c["X"][:6]), np.array(c["noise"][:6])
    Xh[1, 77] = complex(1.0, np.nan)
    Xh[2, 255] = complex(np.inf, 0.0)
    nh[3, 64 * 64 - 1] = complex(np.nan, 0.0)
    Xh[4] = 0
    X, W0, F1, nz, Xp, nzp = _dev(gpu, Xh, c["W0"], c["F1"], nh, c["X"][:6], c["noise"][:6])
    res = beam_scan_batch(X, W0, F1, K, nz, want_power=True, want_total=True)
    tp, ti, st, tot, pw = _np(res)
    plain = _np(beam_scan_batch(Xp, W0, F1, K, nzp, want_power=True, want_total=True))
    assert st.tolist() == [0, 256, 256, 256, 0, 0] and res.degenerate.cpu().numpy().tolist() == [False, True, True, True, False, False]
    for b in (1, 2, 3):
        assert (tp[b] == 0).all() and (ti[b] == -1).all() and tot[b] == 0
    assert (res.p.cpu().numpy()[1:4] == -1).all() and (res.q.cpu().numpy()[1:4] == -1).all()
    for b in (0, 5):
        assert _same([a[b] for a in (tp, ti, st, tot, pw)], [a[b] for a in plain])
    assert np.array_equal(pw[3, :-1], plain[4][3, :-1])   # (the power row is what the product gives)
    # all-zero x with noise: P = |noise|^2 exactly
    want = nh[4].real ** 2 + nh[4].imag ** 2
    assert np.array_equal(pw[4], want)
    order = np.lexsort((np.arange(want.size), -want))[:K]
    assert np.array_equal(ti[4], order) and np.array_equal(tp[4], want[order])
    # all-zero x without noise: all powers 0, the tie rule gives 0 .. K - 1
    z = _np(beam_scan_batch(X[4:5], W0, F1, K, want_power=True, want_total=True))
    assert z[2][0] == 0 and z[1][0].tolist() == [0, 1, 2, 3] and (z[0] == 0).all() and z[3][0] == 0 and not z[4].any()


def test_guard_regions(gpu):
    """Inputs and outputs inside larger NaN-filled buffers at the odd shape (4, 17, 31, 130, 33, 5): the same
    results as from plain tensors (a read past an input's end would bring a NaN in)."""
    import torch
    from ace_amd import beam_scan_batch
    c = SR.case((4, 17, 31, 130, 33, 5), "random")
    X, W0, F1, nz = _dev(gpu, c["X"], c["W0"], c["F1"], c["noise"])
    want = _np(beam_scan_batch(X, W0, F1, 5, nz, want_power=True, want_total=True))
    G = 64

    def guarded(t):
        real = torch.view_as_real(t)
        buf = torch.full((real.numel() + 2 * G,), float("nan"), dtype=torch.float64, device=gpu)
        buf[G:G + real.numel()] = real.reshape(-1)
        return torch.view_as_complex(buf[G:G + real.numel()].view(real.shape))

    got = _np(beam_scan_batch(guarded(X), guarded(W0), guarded(F1), 5, guarded(nz), want_power=True, want_total=True))
    assert _same(got, want)
