"""The operator setup on a side stream beside init, with its host reads coalesced
(csrc/ace_admm.cpp: admm_setup_run, linops_setup).  It only reorders host-side work: no kernel's
arithmetic changes, so every output (X, Y, iteration counts, status, mu) must be BIT-IDENTICAL with
ACE_SETUP_OVERLAP on (default) and off, and a solve must not see the operators of the solve before
or after it on the same stream and workspace.

Geometry: m = 256, 32 x 32 (the only m the m-space runs support, as in test_gpu_msr.py); batch 512
splits into two sub-batches, batch 48 and 40 run as one (40: a ragged last 16-realisation block).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OFF = {"ACE_SETUP_OVERLAP": "0"}


def _np(r):
    return tuple(t.cpu().numpy() for t in (r.X, r.Y, r.iters, r.status, r.mu))


def _solve(monkeypatch, A, B, X0, env, fixed, *, tx=32, rx=32, maxiter=200, counts=False, **kw):
    """One solve in a fresh workspace; with counts, also the launches per kernel class."""
    import torch
    from ace_amd import infer_admm_batch
    from ace_amd._lib import LIB, KERNEL_CLASSES, check
    from ace_amd.solver import Workspace
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if counts:
        check(LIB.ace_prof_sample(1, 0))
        check(LIB.ace_prof_start(20000))
    r = infer_admm_batch(A, B, X0, tx, rx, maxiter=maxiter, fixed_iters=fixed, workspace=Workspace(), **kw)
    torch.cuda.synchronize()
    n = None
    if counts:
        kt = (C.c_double * len(KERNEL_CLASSES))()
        kn = (C.c_int32 * len(KERNEL_CLASSES))()
        check(LIB.ace_prof_stop(kt, kn))
        n = dict(zip(KERNEL_CLASSES, kn))
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return (_np(r), n) if counts else _np(r)


def _same(a, b):
    for u, v in zip(a, b):
        assert np.array_equal(u, v), (np.abs(u - v).max() if u.dtype.kind in "fc" else "ints differ")


@pytest.fixture(scope="module")
def problems(gpu):
    from ace_amd import synth_problem
    return {b: synth_problem(71, 0, b, 256, 32, 32)[:3] for b in (512, 48, 40)}


@pytest.mark.parametrize("batch,fixed", [(512, True), (48, True), (40, True), (512, False)])
def test_knobs_bit_identical(gpu, monkeypatch, problems, batch, fixed):
    """The serial order (ACE_SETUP_OVERLAP=0) against the default, with m-space runs and without (ACE_MSR=0)."""
    A, B, X0 = problems[batch]
    ref, n0 = _solve(monkeypatch, A, B, X0, OFF, fixed, counts=True)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all()
    for env in ({}, {"ACE_MSR": "0"}):
        got, n1 = _solve(monkeypatch, A, B, X0, env, fixed, counts=True)
        print("batch", batch, "fixed", fixed, env, "m-space runs:", n1["msr"], "(serial:", n0["msr"], ")")
        _same(got, ref)
        assert n1["setup"] == n0["setup"] == 1 and (n1["msr"] == n0["msr"] or "ACE_MSR" in env)
    if fixed:
        assert n0["msr"] > 0   # the horizon is long enough for a run to start
    if not fixed:
        assert (ref[2] < 200).any()


def _pair(gpu):
    from ace_amd import synth_problem
    return [synth_problem(seed, 0, 512, 256, 32, 32)[:3] for seed in (81, 82)]


def test_back_to_back_different_codebooks(gpu, monkeypatch):
    """Two solves with different codebooks on one stream and workspace, nothing between them: the
    second setup must not rewrite operators the first solve still reads, and the first solve's
    tail must not read the second's."""
    import torch
    from ace_amd import infer_admm_batch
    from ace_amd.solver import Workspace
    P = _pair(gpu)
    assert not torch.equal(P[0][0], P[1][0])
    alone = [_solve(monkeypatch, *p, {}, True, maxiter=120) for p in P]
    ws = Workspace()
    torch.cuda.synchronize()
    outs = [infer_admm_batch(*p, 32, 32, maxiter=120, fixed_iters=True, workspace=ws) for p in P]
    torch.cuda.synchronize()
    for o, a in zip(outs, alone):
        _same(_np(o), a)


def test_side_stream_pair_is_stream_ordered(gpu, monkeypatch):
    """The same pair on a non-default torch stream, then a torch op on that stream that depends on
    the second result, with no synchronisation in between."""
    import torch
    from ace_amd import infer_admm_batch
    from ace_amd.solver import Workspace
    P = _pair(gpu)
    alone = [_solve(monkeypatch, *p, {}, True, maxiter=120) for p in P]
    ws = Workspace()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        outs = [infer_admm_batch(*p, 32, 32, maxiter=120, fixed_iters=True, workspace=ws, stream=s) for p in P]
        dep = outs[1].X.abs().sum(dim=1) + outs[0].X.abs().sum(dim=1)
    s.synchronize()
    for o, a in zip(outs, alone):
        _same(_np(o), a)
    # (the same device reduction over the finished results: bit-equal unless `dep` ran too early)
    want = outs[1].X.abs().sum(dim=1) + outs[0].X.abs().sum(dim=1)
    torch.cuda.synchronize()
    assert torch.equal(dep, want)


def test_generic_and_private_unchanged(gpu, monkeypatch):
    """A shared A that is no phase code (f64 applies, K Y0 behind the join) and private codebooks
    (serial setup): the knobs change nothing."""
    import torch
    from ace_amd import synth_problem
    g = torch.Generator(device="cpu").manual_seed(5)
    Ag = (torch.randn(1, 64, 256, 2, generator=g, dtype=torch.float64) / 16.0)
    Ag = torch.view_as_complex(Ag).to(gpu)
    A, B, X0, _ = synth_problem(91, 0, 64, 64, 16, 16, A=Ag)
    ref = _solve(monkeypatch, A, B, X0, OFF, True, tx=16, rx=16, maxiter=60)
    assert np.isfinite(ref[0]).all()
    _same(_solve(monkeypatch, A, B, X0, {}, True, tx=16, rx=16, maxiter=60), ref)
    A, B, X0, _ = synth_problem(92, 0, 32, 64, 16, 16, a_shared=False)
    ref = _solve(monkeypatch, A, B, X0, OFF, True, tx=16, rx=16, maxiter=60)
    assert np.isfinite(ref[0]).all()
    _same(_solve(monkeypatch, A, B, X0, {}, True, tx=16, rx=16, maxiter=60), ref)
