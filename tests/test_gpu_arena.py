"""Every asynchronous ``*_batch`` entry against the memory it is given (tests/arena.py): its outputs must not depend
on what its workspace or the bytes around its buffers hold, and it must write nothing outside them.

Per case (arena.run_independent): the control (the same arena and fill twice, bit-identical), the fills 0x00 and
0xFF (the library's ACE_POISON pattern: NaN doubles, -1 ints) over the workspace and every guard band, a predecessor
that leaves another entry's data in the same workspace (default: the scenario generator at ``private_5x20``; the
scenario cases take a PhaseLift solve), the guard bands after every run, and the 0xFF run with the workspace 8, 16
and 248 bytes past a 512-byte boundary.  Every comparison is on the raw bytes of the outputs: no tolerance.  The
inputs (and, for the two wrappers that take ``out=``, the outputs) are arena views at 512-byte alignment between
4 KiB guard bands; the other wrappers' outputs are torch allocations the wrapper makes itself.

What this cannot see: a read past an input that does not change the result (e.g. a vector load whose extra lanes are
masked afterwards) -- a guard band shows writes, and reads only through the outputs.

Shapes are the smallest at which each entry's paths differ, taken from the entries' own test and reference modules.
One line per case: entry, case, workspace bytes, the steps that ran.
"""
import functools

import numpy as np
import pytest

import arena
from arena import OFFSETS, run_independent

pytestmark = pytest.mark.gpu


def _t(gpu, a):
    import torch
    return a.to(gpu) if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a)).to(gpu)   # (a copy: shared inputs are read-only)


def _scenario_pred(ws):
    """The default predecessor: the scenario generator at private_5x20 through ``ws``."""
    import test_gpu_scenario as TS
    TS._run("private_5x20", want=("B", "X0"), workspace=ws)


def _phaselift_pred(ws):
    import torch
    import test_gpu_phaselift as TP
    from ace_amd import phaselift_batch
    Phi, b = TP._problem(7, 4, 40, 2)
    phaselift_batch(torch.from_numpy(Phi).cuda(), torch.from_numpy(b).cuda(), maxIts=3, workspace=ws)
    torch.cuda.synchronize()


def _check(gpu, label, call, inputs, *, outs=None, workspace=True, predecessor=_scenario_pred, offsets=OFFSETS,
           nan_ok=()):
    if not workspace:
        predecessor, offsets = None, ()
    rep = run_independent(call, label=label, device=gpu, inputs={k: _t(gpu, v) for k, v in inputs.items()}, outs=outs,
                          workspace=workspace, predecessor=predecessor, offsets=offsets, nan_ok=nan_ok)
    print(rep.line())
    assert rep.ok, rep.line()
    want = ["control", "fill", "bounds"] if not workspace else ["control", "fill", "history", "alignment", "bounds"]
    assert rep.steps == want, rep.line()
    return rep


# ------------------------------------------------------------------------------------------------ infer_admm_batch
def _admm_case(gpu, label, A, B, X0, tx, rx, **kw):
    import torch
    from ace_amd import BatchResult, infer_admm_batch
    batch, m = B.shape
    n = X0.shape[-1]
    R = 1 if X0.dim() == 2 else (X0.shape[1] if kw.get("scale_by_row", True) else 1)
    shp = (batch,) if X0.dim() == 2 else (batch, R)
    outs = dict(X=(shp + (n,), torch.complex128), Y=(shp + (m,), torch.complex128), iters=((batch,), torch.int32),
                status=((batch,), torch.int32), mu=((batch,), torch.float64))

    def call(inp, ws, out):
        o = BatchResult(out["X"], out["Y"], out["iters"], out["status"], out["mu"])
        r = infer_admm_batch(inp["A"], inp["B"], inp["X0"], tx, rx, out=o, workspace=ws, **kw)
        assert r.X is out["X"]
        return dict(X=r.X, Y=r.Y, iters=r.iters, status=r.status, mu=r.mu)

    return _check(gpu, f"infer_admm_batch {label}", call, dict(A=A, B=B, X0=X0), outs=outs)


@pytest.mark.parametrize("msr", ["1", "0"])
def test_admm_unit_path(gpu, monkeypatch, msr):
    """Batch 40 at m = 256, 32 x 32 (test_gpu_setup_overlap.py: a ragged last 16-realisation block; 120 iterations:
    the m-space runs start), with the runs and with ACE_MSR=0."""
    from ace_amd import synth_problem
    if msr == "0":
        monkeypatch.setenv("ACE_MSR", "0")
    A, B, X0, _ = synth_problem(71, 0, 40, 256, 32, 32)
    _admm_case(gpu, f"unit 40x256x1024 ACE_MSR={msr}", A, B, X0, 32, 32, maxiter=120, fixed_iters=True)


def test_admm_generic_f64_codebook(gpu):
    """The shared codebook that is no phase code of test_generic_and_private_unchanged (64 x 256)."""
    import torch
    from ace_amd import synth_problem
    g = torch.Generator(device="cpu").manual_seed(5)
    Ag = torch.view_as_complex(torch.randn(1, 64, 256, 2, generator=g, dtype=torch.float64) / 16.0).to(gpu)
    A, B, X0, _ = synth_problem(91, 0, 64, 64, 16, 16, A=Ag)
    _admm_case(gpu, "generic f64 64x64x256", A, B, X0, 16, 16, maxiter=60, fixed_iters=True)


@pytest.mark.parametrize("tx,m,batch,seed", [(16, 64, 32, 92), (6, 20, 5, 29)])
def test_admm_private_codebooks(gpu, tx, m, batch, seed):
    """Private codebooks: m = 64, 16 x 16 (test_generic_and_private_unchanged) and (tx, m) = (6, 20), no multiple of
    the code-image tiles (test_gpu_private.py)."""
    from ace_amd import synth_problem
    A, B, X0, _ = synth_problem(seed, 0, batch, m, tx, tx, a_shared=False)
    _admm_case(gpu, f"private {batch}x{m}x{tx * tx}", A, B, X0, tx, tx, maxiter=60, fixed_iters=True)


@functools.lru_cache(maxsize=None)
def _config(which):
    """(A, B, X0) of BASELINE config 3 (test_gpu_parity.py) or 5 (test_gpu_config5.py) at batch 17."""
    if which == 3:
        from ace_amd import synth_problem
        return synth_problem(71, 0, 17, 256, 32, 32)[:3]
    import test_gpu_config5 as T5
    return T5._workload(17)[:3]


@pytest.mark.parametrize("which,r,row", [(3, 1, True), (5, 1, True), (3, 20, True), (5, 20, False)])
def test_admm_configs_3_and_5(gpu, which, r, row):
    """A2nuclear on the codebooks of configs 3 and 5, batch 17, 40 iterations: r = 1 (the m-space iteration) and
    X0 of 20 columns in the row and in the per-column form."""
    import torch
    A, B, X0 = _config(which)
    if r > 1:
        g = torch.Generator(device="cpu").manual_seed(4133 + which)
        X0 = torch.view_as_complex(torch.randn(17, r, 1024, 2, generator=g, dtype=torch.float64) / 16.0)
    _admm_case(gpu, f"config {which} r={r} row={int(row)}", A, B, X0, 32, 32, variant="A2nuclear", scale_by_row=row,
               maxiter=40, fixed_iters=True)


def test_admm_odd_tx(gpu):
    """tx = 1, rx = 8, m = 64, batch 4: this path pads into buffers of its own and ignores the caller's workspace;
    the outputs and every guard are checked all the same."""
    from ace_amd import synth_problem
    A, B, X0, _ = synth_problem(32, 0, 4, 64, 1, 8)
    _admm_case(gpu, "odd tx 4x64x8", A, B, X0, 1, 8, variant="A2only")


# -------------------------------------------------------------------------------------------------------- pipeline
@pytest.mark.parametrize("seed,count", [(41, 6), (61, 17)])
@pytest.mark.parametrize("restarts", [1, 3], ids=["V4", "V4-multi"])
def test_pipeline(gpu, seed, count, restarts):
    """synth.problem(41, 0, 6, 64, 16, 16) and the 17-realisation problem of test_gpu_pipeline.py, with one restart
    (inferLowRankV4) and three (inferLowRankV4_multi)."""
    from ace_amd import draw_partitions, infer_low_rank_pipeline_batch, synth
    A, B, _, _ = synth.problem(seed, 0, count, 64, 16, 16)
    tr = draw_partitions(np.random.default_rng(seed), 64, restarts)

    def call(inp, ws, out):
        r = infer_low_rank_pipeline_batch(inp["A"], inp["B"], 16, 16, tr, workspace=ws)
        return dict(X=r.X, Y=r.Y, quality=r.quality, stage_iters=r.stage_iters, status=r.status)

    _check(gpu, f"pipeline {count}x64x256 restarts={restarts}", call, dict(A=A[0], B=B))


# ------------------------------------------------------------------------------------------------------- PhaseLift
@pytest.mark.parametrize("tx,m,its,blk", [(4, 40, 40, None), (8, 40, 40, None), (8, 40, 40, "1")])
def test_phaselift(gpu, monkeypatch, tx, m, its, blk):
    """(4, 40): m > n, unreduced; (8, 40): reduced, with the default two-stage reduction and with ACE_HETRD_BLK=1."""
    import test_gpu_phaselift as TP
    from ace_amd import phaselift_batch
    if blk is not None:
        monkeypatch.setenv("ACE_HETRD_BLK", blk)
    Phi, b = TP._problem(3 + tx, tx, m, 3)

    def call(inp, ws, out):
        r = phaselift_batch(inp["Phi"], inp["b"], maxIts=its, workspace=ws)
        return dict(sig=r.sig, iters=r.iters, status=r.status)

    _check(gpu, f"phaselift_batch tx={tx} m={m} ACE_HETRD_BLK={blk}", call, dict(Phi=Phi, b=b))


# ---------------------------------------------------------------------------------------------------- GAMP, PR-GAMP
@pytest.mark.parametrize("name,optset,max_em", [("1x5", "plgamp", 200), ("16x16", "cs", 200)])
def test_gamp(gpu, name, optset, max_em):
    """The two smallest shapes of GR.CASES: 1x5 (2 realisations: a partial 16-realisation group) and 16x16."""
    import gamp_ref as GR
    from ace_amd import embgamp_batch
    assert (name, optset, max_em) in GR.CASES
    c = GR.case(name, optset, max_em)

    def call(inp, ws, out):
        r = embgamp_batch(inp["D"], inp["Y"], c["snr"], c["lam"], trace=True, want_xvar=True, workspace=ws, **c["kw"])
        return dict(xhat=r.xhat, params=r.params, em_iters=r.em_iters, status=r.status, trace=r.trace, xvar=r.xvar)

    _check(gpu, f"embgamp_batch {name} {optset}", call, dict(D=c["D"], Y=c["Y"]))


@pytest.mark.parametrize("name,horizon", [("1x5", "handle"), ("16x16", "short")])
def test_prgamp(gpu, name, horizon):
    """The two smallest shapes of PR.CASES: 1x5 (2 realisations: a partial group) and 16x16."""
    import prgamp_ref as PR
    from ace_amd import prgamp_batch
    assert (name, horizon) in PR.CASES
    c = PR.case(name, horizon)

    def call(inp, ws, out):
        r = prgamp_batch(inp["D"], inp["Y"], c["lam"], draws=inp["G"], trace=True, workspace=ws, **c["kw"])
        return dict(xhat=r.xhat, info=r.info, counts=r.counts, status=r.status, trace=r.trace, vals=r.vals)

    _check(gpu, f"prgamp_batch {name} {horizon}", call, dict(D=c["D"], Y=c["Y"], G=c["G"]))


# ------------------------------------------------------------------------------------------------------------- OMP
def test_omp_shapes_bracket_the_threshold():
    import omp_ref as OR
    assert (3, 5, 7, 5) in OR.SHAPES and min(s[1:] for s in OR.SHAPES if s[2] >= 300) == (64, 300, 16)


@pytest.mark.parametrize("shape", [(3, 5, 7, 5), (17, 64, 300, 16)], ids=["3x5x7x5", "17x64x300x16"])
def test_omp(gpu, shape):
    """(3, 5, 7, 5), and the smallest (d, N, kmax) of OR.SHAPES with N >= 300 at 17 realisations (a partial second
    16-realisation block), with colscale and the dense x."""
    import omp_ref as OR
    from ace_amd import omp_batch
    D, Y, w, kmax = OR._inputs(shape)

    def call(inp, ws, out):
        r = omp_batch(inp["D"], inp["Y"], kmax, 0.0, inp["w"], want_x=True, workspace=ws)
        return dict(idx=r.idx, coef=r.coef, count=r.count, resnorm=r.resnorm, status=r.status, x=r.x)

    _check(gpu, "omp_batch " + "x".join(map(str, shape)), call, dict(D=D, Y=Y, w=w))


# ---------------------------------------------------------------------------------------------------------- min-L2
@pytest.mark.parametrize("n,m,mode", [(5, 17, "col"), (16, 48, "row")])
def test_minl2_stage(gpu, n, m, mode):
    import minl2_ref as R
    from ace_amd import minl2_admm_batch
    sbr, cols, maxiter = R.MODES[mode]
    A, B, X0, _ = R.problem(n, m)
    X0 = X0 if cols is None else X0[:, :cols]

    def call(inp, ws, out):
        r = minl2_admm_batch(inp["A"], inp["B"], inp["X0"], scale_by_row=sbr, maxiter=maxiter, want_xall=True,
                             workspace=ws)
        return dict(X=r.X, Y=r.Y, iters=r.iters, objcol=r.objcol, opt_obj=r.opt_obj, mu=r.mu, status=r.status,
                    Xall=r.Xall)

    _check(gpu, f"minl2_admm_batch n={n} m={m} {mode}", call, dict(A=A, B=B, X0=X0))


def test_minl2_recovery(gpu):
    """The whole recovery at n = 16, m = 48 (46 train rows, 2 test rows; the library's own partition)."""
    import minl2_ref as R
    from ace_amd import infer_min_l2_batch
    A, B, _, _ = R.problem(16, 48)

    def call(inp, ws, out):
        r = infer_min_l2_batch(inp["A"], inp["B"], workspace=ws)
        return dict(X=r.X, Y=r.Y, quality=r.quality, stage_iters=r.stage_iters, r_used=r.r_used, status=r.status)

    _check(gpu, "infer_min_l2_batch n=16 m=48", call, dict(A=A, B=B))


# ----------------------------------------------------------------------------------------------------------- A-opt
def _aopt(gpu, label, F, nrows, init):
    from ace_amd import design

    def call(inp, ws, out):
        r = design.aopt_select_batch(inp["F"], inp["nrows"], inp["init"], want_minv=True, workspace=ws)
        return dict(rowlist=r.rowlist, acrit=r.acrit, iters=r.iters, switches=r.switches, status=r.status, Minv=r.Minv)

    _check(gpu, f"aopt_select_batch {label}", call, dict(F=F, nrows=np.asarray(nrows, np.int32),
                                                         init=np.asarray(init, np.int32)))


@pytest.mark.parametrize("which", ["RAGGED", "16x64x24"])
def test_aopt_single_design(gpu, which):
    import test_gpu_aopt as TA
    shape = TA.RAGGED if which == "RAGGED" else (16, 64, 24, 2)
    assert which == "RAGGED" or shape in TA.SHAPES
    F, init = TA.make(*shape)
    _aopt(gpu, which, F, [shape[2]], init[None])


def test_aopt_ten_ragged_designs(gpu):
    """The ten-design batch of test_batch_invariance: ragged row counts over two tile groups."""
    import test_gpu_aopt as TA
    F, nrows, init, _, _ = TA.ragged_designs()
    _aopt(gpu, "ten ragged designs", F, nrows, init)


# -------------------------------------------------------------------------------------------------------- scenario
@pytest.mark.parametrize("name", ["rician_17x33", "combiner_3x9", "private_5x20"])
def test_scenario(gpu, name):
    import test_gpu_scenario as TS
    from ace_amd import scenario_batch
    count, m, tx, rx, shared, _, _ = TS.CASES[name]
    A, W = TS._inputs(name)
    inputs = dict(A=A) if W is None else dict(A=A, W=W)

    def call(inp, ws, out):
        r = scenario_batch(TS.SEED, TS.FIRST, count, tx, rx, inp["A"], TS._cfg(name), inp.get("W"), want=TS.OUTS,
                           workspace=ws, a_shared=shared)
        return {k: getattr(r, k) for k in TS.OUTS}

    _check(gpu, f"scenario_batch {name}", call, inputs, predecessor=_phaselift_pred)


# ------------------------------------------------------------------------------------ entries without a workspace
def test_evaluate(gpu):
    import eval_ref as ER
    import test_gpu_evaluate as TE
    from ace_amd import evaluate_batch
    tx, rx = sorted(TE.SHAPES)[1]   # (2, 3): the smallest shape past 1 x 1
    X, G = ER.seeded_problem(1000 * tx + rx, 3, tx, rx)

    def call(inp, ws, out):
        r = evaluate_batch(inp["X"], inp["G"], tx, rx)
        return dict(metrics=r.metrics, status=r.status)

    _check(gpu, f"evaluate_batch {tx}x{rx}", call, dict(X=X, G=G), workspace=False)


def test_evaluate_rss(gpu):
    import rss_ref as RR
    from ace_amd import evaluate_rss_batch
    shape = RR.SHAPES[2]   # (3, 9, 5): the smallest shape with more than one of everything
    c = RR.case(*shape, "random")

    def call(inp, ws, out):
        r = evaluate_rss_batch(inp["X"], inp["CB"], inp["rss"], want_pred=True)
        return dict(metrics=r.metrics, status=r.status, pred=r.pred)

    _check(gpu, "evaluate_rss_batch " + "x".join(map(str, shape)), call, dict(X=c["X"], CB=c["CB"], rss=c["rss"]),
           workspace=False)


def test_beam_scan(gpu):
    import scan_ref as SR
    from ace_amd import beam_scan_batch
    shape = SR.SHAPES[1]   # (3, 3, 5, 7, 2, 3): the smallest shape with more than one of everything
    c = SR.case(shape, "random")

    def call(inp, ws, out):
        r = beam_scan_batch(inp["X"], inp["W0"], inp["F1"], c["K"], inp["noise"], want_power=True, want_total=True)
        return dict(top_pow=r.top_pow, top_idx=r.top_idx, status=r.status, total=r.total, power=r.power)

    _check(gpu, "beam_scan_batch " + "x".join(map(str, shape)), call,
           dict(X=c["X"], W0=c["W0"], F1=c["F1"], noise=c["noise"]), workspace=False)


def test_beamformer(gpu):
    from ace_amd import svd_beamformer_batch
    rng = np.random.default_rng(13)
    H = rng.standard_normal((5, 1, 8)) + 1j * rng.standard_normal((5, 1, 8))   # (1, 8): the smallest of RECT

    def call(inp, ws, out):
        r = svd_beamformer_batch(inp["H"], want_vh=True)
        return dict(wr=r.wr_code, wt=r.wt_code, idx=r.beam_idx, rss=r.rss, status=r.status, vh_r=r.vh_r, vh_t=r.vh_t)

    _check(gpu, "svd_beamformer_batch 5x1x8", call, dict(H=H), workspace=False)


def test_synth_problem(gpu):
    """The generator writes A, B, X0 and H itself; with a caller's codebook A is its one input."""
    from ace_amd import synth, synth_problem
    A = synth.codebook(11, 20, 24)[None]

    def call(inp, ws, out):
        _, B, X0, H = synth_problem(11, 0, 3, 20, 6, 4, A=inp["A"])
        return dict(B=B, X0=X0, H=H)

    _check(gpu, "synth_problem 3x20x24", call, dict(A=A), workspace=False)


@pytest.mark.parametrize("tau", [1.0, 0.75])
def test_nuclear_prox_after_a_solve(gpu, tau):
    """nuclear_prox_batch takes its scratch from the stream-ordered pool: the control and the bounds (E, and Z through
    out=), then the call again right after an ADMM solve on the same stream -- the same bits."""
    import torch
    from ace_amd import infer_admm_batch, nuclear_prox_batch, synth_problem
    n, r = 64, 7   # (tests/test_svt_kat.py)
    rng = np.random.default_rng(3)
    E = (rng.standard_normal((5, r, n)) + 1j * rng.standard_normal((5, r, n))) / np.sqrt(n)
    E[1] = E[1, :1].repeat(r, axis=0) * np.linspace(1, 2, r)[:, None]     # rank one

    def call(inp, ws, out):
        return dict(Z=nuclear_prox_batch(inp["E"], tau, out=out["Z"]))

    _check(gpu, f"nuclear_prox_batch 5x{r}x{n} tau={tau}", call, dict(E=E), outs=dict(Z=((5, r, n), torch.complex128)),
           workspace=False)
    Ed = _t(gpu, E)
    ref = arena.raw_bytes(nuclear_prox_batch(Ed, tau))
    A, B, X0, _ = synth_problem(5, 0, 8, 64, 16, 16)
    infer_admm_batch(A, B, X0, 16, 16, maxiter=20, fixed_iters=True)
    got = nuclear_prox_batch(Ed, tau)          # (no synchronisation in between: the same stream)
    torch.cuda.synchronize()
    assert np.array_equal(arena.raw_bytes(got), ref) and not np.isnan(got.cpu().numpy()).any()
    print(f"arena nuclear_prox_batch tau={tau}: history (after an ADMM solve on the stream) ok")


# ---------------------------------------------------------------------------------------------- odd-tx regression
ODD_TX_SEQUENCE = [(1, 8, 32), (2, 8, 32), (2, 4, 32), (1, 8, 64), (1, 8, 64), (2, 4, 64), (1, 8, 64)]


def test_odd_tx_sequence(gpu):
    """The order of solves in one process that once made the Newton-Schulz setup of the tx = 1, m = 64 A2only solve
    fail when its buffers came from the stream-ordered pool.  Through the host entry, and through
    the device entry on one shared workspace filled with 0xFF beforehand: every solve returns, the three (1, 8, 64)
    solves are bit-identical, and the device results equal the host results bit for bit."""
    import torch
    from ace_amd import infer_admm_batch, infer_admm_host, synth
    from ace_amd.solver import Workspace
    probs = [synth.problem(31 + tx, 0, 4, m, tx, rx) for tx, rx, m in ODD_TX_SEQUENCE]
    host = [infer_admm_host(A, B, X0, tx, rx, variant="A2only") for (tx, rx, m), (A, B, X0, _) in zip(ODD_TX_SEQUENCE, probs)]
    ws = Workspace()
    ws.buf = torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=gpu)
    view = ws.buf
    dev = []
    for (tx, rx, m), (A, B, X0, _) in zip(ODD_TX_SEQUENCE, probs):
        r = infer_admm_batch(_t(gpu, A), _t(gpu, B), _t(gpu, X0), tx, rx, variant="A2only", workspace=ws)
        torch.cuda.synchronize()
        dev.append(r)
    assert ws.buf is view   # (every solve ran in the poisoned workspace)
    fields = ("X", "Y", "iters", "status", "mu")
    for h, d, c in zip(host, dev, ODD_TX_SEQUENCE):
        for k in fields:
            hv, dv = getattr(h, k), getattr(d, k).cpu().numpy()
            assert np.array_equal(arena.raw_bytes(hv), arena.raw_bytes(dv)), (c, k)
        assert np.isfinite(h.X).all() and np.isfinite(h.Y).all(), c
    same = [i for i, c in enumerate(ODD_TX_SEQUENCE) if c == (1, 8, 64)]
    assert len(same) == 3
    for i in same[1:]:
        for k in fields:
            assert np.array_equal(arena.raw_bytes(getattr(host[i], k)), arena.raw_bytes(getattr(host[same[0]], k))), (i, k)
