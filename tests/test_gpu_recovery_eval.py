"""GPU tests of the batched sparse-recovery evaluator (ace_evaluate_recovery_*: Evaluation_Recovery.m:73-338 on the
device).

Target: the numpy restatement tests/recovery_ref.py on seeded inputs of three kinds (dense like GAMP's output,
L-sparse with exact zeros like OMP's, the largest entries in the first and the last atom of the cut grid).  Bars:
Num_Quantization_Error exact; the three angle errors 1e-10 degrees; MSE_ARM 1e-10; MSE_H and proj_error absolute 1e-9
and the two gains 1e-9 ||H||_F (tests/test_gpu_evaluate.py's bars); each rate that gain bar propagated through
|log2(1 + L g^2 / sigma^2)| at the restatement's own gain g, (2 |g| / ((sigma^2 + L g^2) ln 2)) L 1e-9 ||H||_F + 1e-12.
The columns that quantise phases leave out the realisations the restatement flags as within 1e-6 rad of a
quantisation boundary; at most 2 % of a shape's realisations may be flagged.
"""
import functools
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import recovery_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu

# (tx, rx, NQ_t, NQ_r, search_deg, L)
SHAPES = [(1, 4, 4, 16, 120.0, 1), (4, 4, 16, 16, 120.0, 1), (8, 4, 25, 16, 40.0, 1), (12, 12, 48, 48, 40.0, 1),
          (16, 16, 64, 64, 120.0, 1), (16, 16, 64, 64, 120.0, 3), (32, 32, 128, 128, 180.0, 2)]
IDS = [f"{s[0]}x{s[1]}-g{s[2]}x{s[3]}-{int(s[4])}deg-L{s[5]}" for s in SHAPES]
BATCHES = [1, 3, 65]
NP = 0.1          # noise power
M_SWEEP = (5, 3)  # (Mt, Mr) of the sweep tables
ANGLE_BAR, ARM_BAR, ABS_BAR, GAIN_BAR = 1e-10, 1e-10, 1e-9, 1e-9
ANGLE_COLS, RATE_COLS = (1, 10, 11), (4, 5, 6, 7, 8, 9)


@functools.lru_cache(maxsize=None)
def _problem(shape):
    """65 seeded realisations of a shape with the restatement's metrics: computed once, shared, never modified."""
    from ace_amd import angular, recovery_tables
    from ace_amd.recovery_eval import SweepTables
    tx, rx, NQ_t, NQ_r, deg, L = shape
    tb = recovery_tables(tx, rx, NQ_t, NQ_r, deg)
    Z, H, aod, aoa, tidx = RR.seeded_problem(7000 + 100 * tx + rx + L, max(BATCHES), tb, L, deg)
    Ft, cen_t = angular.directional_beams(tx, M_SWEEP[0], deg)
    Wr, cen_r = angular.directional_beams(rx, M_SWEEP[1], deg)
    grid = angular.peak_angle_grid()
    sw = SweepTables(cen_t, cen_r, RR.peak_angles(Ft, tb.kappa, grid)[0], RR.peak_angles(Wr, tb.kappa, grid)[0])
    rng = np.random.default_rng(11)
    picks = np.stack([rng.integers(0, M_SWEEP[0], (len(Z), 2)), rng.integers(0, M_SWEEP[1], (len(Z), 2))],
                     axis=-1).astype(np.int32)   # [batch][pattern][(ind_F, ind_W)]
    met, He, nb = RR.evaluate(Z, H, aod, aoa, tb, tidx, NP, picks, sw)
    for a in (Z, H, aod, aoa, tidx, picks, met, He, nb):
        a.setflags(write=False)
    return tb, sw, Z, H, aod, aoa, tidx, picks, met, He, nb


def _check(got, exp, H, nb, L, what):
    """The parity bars, column by column; prints each column's largest deviation over its bar's unit."""
    gn = np.linalg.norm(H, axis=1)
    dev = np.abs(got - exp)
    bar = np.empty_like(dev)
    bar[:, 0] = 0.0
    bar[:, ANGLE_COLS] = ANGLE_BAR
    bar[:, 2] = ARM_BAR
    bar[:, (3, 14)] = ABS_BAR
    bar[:, (12, 13)] = GAIN_BAR * gn[:, None]
    for c in RATE_COLS:
        g = RR.gains_of(exp[:, c], L, NP)
        bar[:, c] = 2 * g / ((NP + L * g * g) * np.log(2)) * L * GAIN_BAR * gn + 1e-12
    for c in RR.QUANTISED:
        dev[nb, c] = 0.0
    over = dev > bar
    worst = (dev / np.where(bar > 0, bar, 1.0)).max(axis=0)
    print(f"{what}: largest deviation over its bar per column {np.array2string(worst, precision=2)} "
          f"({int(nb.sum())} near-boundary left out of columns {RR.QUANTISED})")
    assert not over.any(), (what, np.argwhere(over)[:8], dev[over][:8], bar[over][:8])


def _host(shape, rows, sweep=True, want_H_est=False):
    from ace_amd import evaluate_recovery_host
    tb, sw, Z, H, aod, aoa, tidx, picks = _problem(shape)[:8]
    return evaluate_recovery_host(Z[rows], H[rows], aod[rows], aoa[rows], tb, noise_power=NP, true_idx=tidx[rows],
                                  picks=picks[rows] if sweep else None, sweep=sw if sweep else None,
                                  want_H_est=want_H_est)


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_the_numpy_restatement(gpu, shape, batch):
    H, met, nb = _problem(shape)[3], _problem(shape)[8], _problem(shape)[10]
    assert nb.mean() <= 0.02, (shape, int(nb.sum()))
    # batch 1: each kind of z alone (rows 0, 1, 2 are dense, L-sparse, edge)
    for rows in ([slice(0, batch)] if batch > 1 else [slice(k, k + 1) for k in range(3)]):
        res = _host(shape, rows)
        assert (res.status == 0).all() and not res.degenerate.any() and not res.no_sweep.any()
        assert np.isfinite(res.metrics).all()
        np.testing.assert_array_equal(res.metrics[:, 3], res.mse_h)
        np.testing.assert_array_equal(res.metrics[:, 14], res.proj_error)
        _check(res.metrics, met[rows], H[rows], nb[rows], shape[5], f"{shape} rows {rows}")


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[5], SHAPES[6]], ids=[IDS[2], IDS[5], IDS[6]])
def test_h_est_and_the_last_three_columns_against_the_channel_evaluator(gpu, shape):
    """H_est is AD z after the global phase; columns 12-14 are evaluate(H_est, H) with the receive side leading."""
    from ace_amd import evaluate_host
    tx, rx = shape[:2]
    H, He = _problem(shape)[3], _problem(shape)[9]
    res = _host(shape, slice(0, 65), want_H_est=True)
    scale = np.abs(He).max(axis=1, keepdims=True)
    assert (np.abs(res.H_est - He) <= 1e-12 * scale).all(), np.abs(res.H_est - He).max()
    ev = evaluate_host(res.H_est, H, rx, tx)
    gn = np.linalg.norm(H, axis=1)
    assert (ev.status == 0).all()
    assert (np.abs(ev.gain_ana - res.gain_ana) <= GAIN_BAR * gn).all()
    assert (np.abs(ev.gain_dig - res.gain_dig) <= GAIN_BAR * gn).all()
    assert (np.abs(ev.proj_err - res.proj_error) <= ABS_BAR).all()


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[5], SHAPES[6]], ids=[IDS[0], IDS[5], IDS[6]])
def test_batch_invariance(gpu, shape):
    """Row k of a batch of 65 is bit-identical to the same row evaluated alone."""
    full = _host(shape, slice(0, 65), want_H_est=True)
    for k in (0, 1, 2, 37, 64):
        one = _host(shape, slice(k, k + 1), want_H_est=True)
        assert np.array_equal(one.metrics[0], full.metrics[k]), k
        assert one.status[0] == full.status[k] and np.array_equal(one.H_est[0], full.H_est[k])


def test_degenerate_rows(gpu):
    """Row 1 of z zero, row 2 with a NaN, row 3 of H zero, row 4 of H with an Inf: the flag and the stated values
    (the angle columns of a degenerate z are those of the picks 0 .. L - 1); every other row is untouched, bit for bit."""
    from ace_amd import evaluate_recovery_host
    from ace_amd._lib import ACE_ST_EVAL_DEGENERATE
    shape = SHAPES[5]
    tb, sw, Z, H, aod, aoa, tidx, picks = _problem(shape)[:8]
    L = shape[5]
    Z, H = Z[:7].copy(), H[:7].copy()
    kw = dict(noise_power=NP, true_idx=tidx[:7], picks=picks[:7], sweep=sw, want_H_est=True)
    clean = evaluate_recovery_host(Z, H, aod[:7], aoa[:7], tb, **kw)
    Z[1] = 0.0
    Z[2, 17] = complex(np.nan, 0.0)
    H[3] = 0.0
    H[4, 5] = complex(0.0, -np.inf)
    res = evaluate_recovery_host(Z, H, aod[:7], aoa[:7], tb, **kw)
    assert res.degenerate.tolist() == [False, True, True, True, True, False, False]
    assert (res.status[1:5] == ACE_ST_EVAL_DEGENERATE).all() and (res.status[[0, 5, 6]] == 0).all()
    for b in range(1, 5):
        m = res.metrics[b]
        assert m[2] == 1.0 and m[3] == 1.0 and m[14] == 1.0 and (m[4:10] == 0.0).all() and (m[12:14] == 0.0).all()
        assert m[0] == 0.0 and np.isfinite(m[[1, 10, 11]]).all()
        assert (res.H_est[b] == 0.0).all()
        assert np.array_equal(m[[10, 11]], clean.metrics[b, [10, 11]])   # the sweep's errors need no z and no H
    for b in (3, 4):
        assert res.metrics[b, 1] == clean.metrics[b, 1]                  # a good z keeps its own picks
    # picks 0 .. L - 1 are atoms (0, 0 .. L - 1): AoD estimates all deg_t[0], AoA estimates deg_r[0 .. L - 1]
    tD = np.sort(aod[1])[::-1]
    exp = (np.mean(np.abs(tb.deg_t[0] - tD)) + np.mean(np.abs(tb.deg_r[:L] - aoa[1]))) / 2
    assert res.metrics[1, 1] == pytest.approx(exp, abs=1e-10)
    for b in (0, 5, 6):
        assert np.array_equal(res.metrics[b], clean.metrics[b])
        assert np.array_equal(res.H_est[b], clean.H_est[b])


def test_no_sweep_picks_give_nan_and_the_status_bit(gpu):
    from ace_amd import evaluate_recovery_host
    from ace_amd._lib import ACE_ST_RECEVAL_NOSWEEP
    shape = SHAPES[3]
    tb, sw, Z, H, aod, aoa, tidx, picks = _problem(shape)[:8]
    with_sw, without = _host(shape, slice(0, 9)), _host(shape, slice(0, 9), sweep=False)
    assert (without.status == ACE_ST_RECEVAL_NOSWEEP).all() and without.no_sweep.all()
    assert np.isnan(without.metrics[:, 8:12]).all()
    rest = [c for c in range(15) if c not in (8, 9, 10, 11)]
    assert np.array_equal(without.metrics[:, rest], with_sw.metrics[:, rest])
    # a row whose pick is the scan's -1 (a degenerate sweep) loses its sweep columns alone
    p = picks[:9].copy()
    p[4, 0, 1] = -1
    p[6, 1, 0] = M_SWEEP[0]
    res = evaluate_recovery_host(Z[:9], H[:9], aod[:9], aoa[:9], tb, noise_power=NP, true_idx=tidx[:9], picks=p, sweep=sw)
    assert res.no_sweep.tolist() == [b in (4, 6) for b in range(9)]
    assert np.isnan(res.metrics[[4, 6], 8:12]).all()
    keep = [b for b in range(9) if b not in (4, 6)]
    assert np.array_equal(res.metrics[keep], with_sw.metrics[keep])


def test_device_entry_on_a_stream_with_out(gpu):
    """evaluate_recovery_batch on a non-default stream into caller-owned, poisoned outputs equals the host entry bit
    for bit, and the rows past the batch keep their poison."""
    import torch
    from ace_amd import evaluate_recovery_batch, RecoveryEval
    shape = SHAPES[2]
    tb, sw, Z, H, aod, aoa, tidx, picks = _problem(shape)[:8]
    B, nh = 33, shape[0] * shape[1]
    host = _host(shape, slice(0, B), want_H_est=True)
    up = lambda a: torch.from_numpy(np.array(a[:B])).to(gpu)  # noqa: E731
    met = torch.full((B + 1, 15), -7.0, dtype=torch.float64, device=gpu)
    st = torch.full((B + 1,), -1, dtype=torch.int32, device=gpu)
    He = torch.full((B + 1, nh), -7.0, dtype=torch.complex128, device=gpu)
    out = RecoveryEval(met[:B], st[:B], He[:B])
    args = [up(Z), up(H), up(aod), up(aoa)]
    dti, dpk = up(tidx), up(picks)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    res = evaluate_recovery_batch(*args, tb, noise_power=NP, true_idx=dti, picks=dpk, sweep=sw, want_H_est=True,
                                  out=out, stream=s)
    s.synchronize()
    assert res.metrics.data_ptr() == met.data_ptr() and res.status.data_ptr() == st.data_ptr()
    assert res.H_est.data_ptr() == He.data_ptr()
    assert np.array_equal(met[:B].cpu().numpy(), host.metrics)
    assert np.array_equal(st[:B].cpu().numpy().view(np.uint32), host.status)
    assert np.array_equal(He[:B].cpu().numpy(), host.H_est)
    assert (met[B] == -7.0).all() and st[B] == -1 and (He[B] == -7.0).all()
    # the nearest true indices computed in torch are the host's
    assert np.array_equal(tb.true_indices(args[2], args[3]).cpu().numpy(), tidx[:B])
    torch.cuda.synchronize()
