"""Sparse-recovery evaluation on the GPU: the reference's ``Evaluation_Recovery``
(Numerical_Simulation/src/evaluate_plot_results/Evaluation_Recovery.m:73-338), batched against one shared pair of cut
steering dictionaries.  It is the score the reference gives the recoveries on the angular dictionary (PLOMP, PLGAMP,
PerfectPhaseCS, NoisyPhaseCS, PRGAMP: Vs_M.m:215-221, Vs_SNR.m:192-194, sub_VS_SR_par.m:166-170); the low-rank
recoveries go through ``evaluate.evaluate_batch`` (Evaluation_H).

Per realisation, from the recovered sparse vector z [Qt*Qr] (index u Qr + v as in ``sparse.dictionary_2d``), the true
channel vecH (element r + rx t), the true angles and, optionally, the two sweep picks, the 15 numbers of :322-336 in
the order ``METRICS_RECOVERY``.  The recovered channel ``AD z`` is never formed as a dense product: the kernel
computes ``A_r^T mat(z)^T conj(A_t)`` on the f64 matrix cores and reads z once (csrc/ace_receval.hip, which also
lists how the reference's quirks are restated).  Columns ``gain_ana``, ``gain_dig``, ``proj_error`` are
``evaluate_batch(H_est, H, rx, tx)``'s.

A realisation whose z or H is all zero or not finite returns mse_h = mse_arm = proj_error = 1, gains and rates 0 and
ACE_ST_EVAL_DEGENERATE; without sweep picks the four sweep columns are NaN and ACE_ST_RECEVAL_NOSWEEP is set.

Entry points (no CPU fallback -- every call runs ``receval_kernel`` on the GPU):
  * ``recovery_tables(tx, rx, NQ_t, NQ_r, search_deg, paths=...)`` -- the per-call tables, built on the host once.
  * ``sweep_tables(tx, rx, Mt, Mr, search_deg)`` -- the two sweep patterns' angle tables (``angular.beam_peak_angles``).
  * ``evaluate_recovery_host(z, vecH, aod_deg, aoa_deg, tables, noise_power=...)`` -- numpy arrays.
  * ``evaluate_recovery_batch(...)`` -- device tensors already in HBM; no host copy.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import angular
from ._lib import LIB, check, ACE_ST_EVAL_DEGENERATE, ACE_ST_RECEVAL_NOSWEEP

# column order of the C-ABI's metrics [batch][15] (Evaluation_Recovery.m:322-336)
METRICS_RECOVERY = ("num_quantization_error", "aoda_err", "mse_arm", "mse_h", "rate_unconstrained", "rate_percsi",
                    "rate_est", "rate_est_aoda", "rate_bsweep1", "rate_bsweep2", "aoda_err_sweep1", "aoda_err_sweep2",
                    "gain_ana", "gain_dig", "proj_error")
NCOL = len(METRICS_RECOVERY)
SWEEP_COLUMNS = (8, 9, 10, 11)
L_MAX, ANT_MAX, Q_MAX = 8, 32, 4096   # the C-ABI's limits (include/ace.h)


@dataclass
class RecoveryEval:
    """``metrics`` [batch][15] float64 (columns ``METRICS_RECOVERY``, each also an attribute), ``status`` [batch]
    uint32 (host) / int32 (device): ACE_ST_EVAL_DEGENERATE, ACE_ST_RECEVAL_NOSWEEP, ACE_ST_BF_NOCONV; ``H_est``
    [batch][tx*rx] complex128 when asked for."""
    metrics: object
    status: object
    H_est: object = None

    def __getattr__(self, name):
        try:
            return self.__dict__["metrics"][:, METRICS_RECOVERY.index(name)]
        except (ValueError, KeyError):
            raise AttributeError(name) from None

    @property
    def degenerate(self):
        return (self.status & ACE_ST_EVAL_DEGENERATE) != 0

    @property
    def no_sweep(self):
        return (self.status & ACE_ST_RECEVAL_NOSWEEP) != 0


@dataclass
class SweepTables:
    """The angle estimates of the reference's two sweep patterns per beam index (degrees): ``centre_deg_*`` pattern
    2's (MyBeamSweeping.m:156-157), ``peak_deg_*`` pattern 1's (:134-154)."""
    centre_deg_t: np.ndarray   # [Mt]
    centre_deg_r: np.ndarray   # [Mr]
    peak_deg_t: np.ndarray     # [Mt]
    peak_deg_r: np.ndarray     # [Mr]


@dataclass
class RecoveryTables:
    """What a call shares among its realisations (host arrays; ``dev`` caches the device copies)."""
    tx: int
    rx: int
    A_t: np.ndarray      # [Qt][tx] complex128, the rows of ``angular.dictionary(tx, NQ_t, search_deg)``
    A_r: np.ndarray      # [Qr][rx]
    deg_t: np.ndarray    # [Qt] the cut grid's angles in degrees (Evaluation_Recovery.m:105-113)
    deg_r: np.ndarray    # [Qr]
    first_t: int         # global (uncut) grid index of column 0 per side
    first_r: int
    grid_t: np.ndarray   # [NQ_t] the uncut sin grid
    grid_r: np.ndarray   # [NQ_r]
    kappa: float         # 2 pi d / lambda
    aod_deg: object = None    # [batch][L] with ``paths``
    aoa_deg: object = None
    true_idx: object = None   # [batch][L][2] int32 with ``paths``
    dev: dict = field(default_factory=dict, repr=False)

    @property
    def Qt(self):
        return len(self.deg_t)

    @property
    def Qr(self):
        return len(self.deg_r)

    def true_indices(self, aod_deg, aoa_deg):
        """[batch][L][2] int32: the global grid index nearest in sin to each true AoD / AoA, the first on a tie
        (Quan_Pos_Err_h_array(2, l, 1:2), Sparse_Channel_Formulation.m:96-103; zero-based).  numpy in, numpy out;
        device tensors in, a device tensor out."""
        if isinstance(aod_deg, np.ndarray):
            near = lambda g, a: np.argmin(np.abs(g[None, None, :] - np.sin(np.deg2rad(a))[..., None]), axis=-1)  # noqa: E731
            return np.ascontiguousarray(np.stack([near(self.grid_t, aod_deg), near(self.grid_r, aoa_deg)], axis=-1)
                                        .astype(np.int32))
        import torch

        def near(g, a):
            g = self._up("grid_" + g, getattr(self, "grid_" + g), a.device)
            d = (g[None, None, :] - torch.sin(torch.deg2rad(a))[..., None]).abs()
            idx = torch.arange(g.shape[0], device=a.device)
            return torch.where(d == d.min(dim=-1, keepdim=True).values, idx, g.shape[0]).min(dim=-1).values
        return torch.stack([near("t", aod_deg), near("r", aoa_deg)], dim=-1).to(torch.int32).contiguous()

    def _up(self, name, a, device):
        import torch
        key = (name, str(device))
        if key not in self.dev:
            self.dev[key] = torch.from_numpy(np.ascontiguousarray(a)).to(device)
        return self.dev[key]


def split_paths(paths, L):
    """(aod_deg [batch][L], aoa_deg [batch][L]) of a scenario's ``paths`` (include/ace.h states the layout)."""
    return paths[:, :L], paths[:, L:2 * L]


def recovery_tables(tx, rx, NQ_t=None, NQ_r=None, search_deg=angular.SEARCH_DEG, paths=None, L=None,
                    ant_d=None) -> RecoveryTables:
    """The per-call tables of ``evaluate_recovery_*`` for the cut dictionaries ``sparse.dictionary_2d(tx, rx, NQ_t,
    NQ_r, search_deg)`` is built from: the dictionaries' rows, their angles in degrees, the global index of the first
    cut column per side.  With a scenario's ``paths`` (numpy or a device tensor; ``L`` dominant paths) the true angles
    and their nearest global grid indices are attached as ``aod_deg``, ``aoa_deg``, ``true_idx``."""
    from . import synth
    NQ_t = 4 * tx if NQ_t is None else int(NQ_t)
    NQ_r = 4 * rx if NQ_r is None else int(NQ_r)
    A_t, _, deg_t = angular.dictionary(tx, NQ_t, search_deg, ant_d)
    A_r, _, deg_r = angular.dictionary(rx, NQ_r, search_deg, ant_d)
    g_t, lo_t, _ = angular.grid_cut(NQ_t, search_deg)
    g_r, lo_r, _ = angular.grid_cut(NQ_r, search_deg)
    kappa = angular.KAPPA if ant_d is None else 2.0 * np.pi * (float(ant_d) / synth.LAMBDA)
    tb = RecoveryTables(int(tx), int(rx), np.ascontiguousarray(A_t), np.ascontiguousarray(A_r),
                        np.ascontiguousarray(deg_t), np.ascontiguousarray(deg_r), lo_t, lo_r, g_t, g_r, float(kappa))
    if paths is not None:
        if L is None:
            raise ValueError("recovery_tables: paths needs L, the number of dominant paths")
        tb.aod_deg, tb.aoa_deg = split_paths(paths, int(L))
        if not isinstance(paths, np.ndarray):
            tb.aod_deg, tb.aoa_deg = tb.aod_deg.contiguous(), tb.aoa_deg.contiguous()
        tb.true_idx = tb.true_indices(tb.aod_deg, tb.aoa_deg)
    return tb


def sweep_tables(tx, rx, Mt, Mr, search_deg=angular.SEARCH_DEG) -> SweepTables:
    """The angle tables of the two sweep patterns over ``angular.directional_beams``: the partition centres and the
    peak angles of the quantised beams (``angular.beam_peak_angles``, on the GPU)."""
    Ft, cen_t = angular.directional_beams(tx, Mt, search_deg)
    Wr, cen_r = angular.directional_beams(rx, Mr, search_deg)
    return SweepTables(np.ascontiguousarray(cen_t), np.ascontiguousarray(cen_r), angular.beam_peak_angles(Ft),
                       angular.beam_peak_angles(Wr))


def _check_shapes(tb, zs, hs, ads, aas, tis, pks, sweep):
    if not isinstance(tb, RecoveryTables):
        raise TypeError("tables must be a RecoveryTables (recovery_tables(...))")
    nz, nh = tb.Qt * tb.Qr, tb.tx * tb.rx
    if len(zs) != 2 or zs[0] < 1 or zs[1] != nz:
        raise ValueError(f"z must be [batch][Qt*Qr] = [batch][{nz}], got {tuple(zs)}")
    batch = zs[0]
    if tuple(hs) != (batch, nh):
        raise ValueError(f"vecH must be [batch][tx*rx] = [{batch}][{nh}], got {tuple(hs)}")
    if len(ads) != 2 or ads[0] != batch or not 1 <= ads[1] <= L_MAX or tuple(aas) != tuple(ads):
        raise ValueError(f"aod_deg and aoa_deg must be [batch][L] with 1 <= L <= {L_MAX}, got {tuple(ads)} and {tuple(aas)}")
    L = ads[1]
    if L > nz:
        raise ValueError(f"L = {L} exceeds the grid's {nz} atoms")
    if tuple(tis) != (batch, L, 2):
        raise ValueError(f"true_idx must be [batch][L][2] = [{batch}][{L}][2], got {tuple(tis)}")
    if (pks is None) != (sweep is None):
        raise ValueError("picks and sweep (a SweepTables) go together")
    if pks is not None and tuple(pks) != (batch, 2, 2):
        raise ValueError(f"picks must be [batch][2][2] = [{batch}][2][2], got {tuple(pks)}")
    return batch, L


def _noise(noise_power):
    noise_power = float(noise_power)
    if not (noise_power > 0.0 and np.isfinite(noise_power)):
        raise ValueError("noise_power must be positive and finite")
    return noise_power


def evaluate_recovery_host(z, vecH, aod_deg, aoa_deg, tables, *, noise_power, true_idx=None, picks=None, sweep=None,
                           want_H_est=False) -> RecoveryEval:
    """Evaluation_Recovery for a batch on host arrays: z [batch][Qt*Qr] and vecH [batch][tx*rx] complex, the true
    angles [batch][L] in degrees, ``tables`` from ``recovery_tables``.  ``true_idx`` [batch][L][2] (default:
    ``tables.true_indices(aod_deg, aoa_deg)``); ``picks`` [batch][2][2] int32 with ``sweep`` (a ``SweepTables``): the
    zero-based (ind_F, ind_W) of sweep pattern 1 and 2."""
    if not isinstance(tables, RecoveryTables):
        raise TypeError("tables must be a RecoveryTables (recovery_tables(...))")
    c = lambda a, t: np.ascontiguousarray(np.asarray(a, dtype=t))  # noqa: E731
    z, vecH = np.atleast_2d(c(z, np.complex128)), np.atleast_2d(c(vecH, np.complex128))
    aod_deg, aoa_deg = np.atleast_2d(c(aod_deg, np.float64)), np.atleast_2d(c(aoa_deg, np.float64))
    true_idx = tables.true_indices(aod_deg, aoa_deg) if true_idx is None else c(true_idx, np.int32)
    picks = None if picks is None else c(picks, np.int32)
    batch, L = _check_shapes(tables, z.shape, vecH.shape, aod_deg.shape, aoa_deg.shape, true_idx.shape,
                             None if picks is None else picks.shape, sweep)
    met = np.empty((batch, NCOL), np.float64)
    st = np.empty(batch, np.uint32)
    He = np.empty((batch, tables.tx * tables.rx), np.complex128) if want_H_est else None
    dp = lambda a: None if a is None else a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    sw = [None] * 4 if sweep is None else [c(getattr(sweep, k), np.float64) for k in
                                           ("centre_deg_t", "centre_deg_r", "peak_deg_t", "peak_deg_r")]
    Mt, Mr = (0, 0) if sweep is None else (len(sw[0]), len(sw[1]))
    if sweep is not None and (len(sw[2]) != Mt or len(sw[3]) != Mr):
        raise ValueError("sweep: the centre and the peak tables of a side must have one length")
    check(LIB.ace_evaluate_recovery_host(batch, tables.tx, tables.rx, L, tables.Qt, tables.Qr, dp(tables.A_t),
                                         dp(tables.A_r), dp(tables.deg_t), dp(tables.deg_r), tables.first_t,
                                         tables.first_r, _noise(noise_power), tables.kappa, dp(z), dp(vecH), dp(aod_deg),
                                         dp(aoa_deg), ip(true_idx), ip(picks), Mt, Mr, *[dp(a) for a in sw], dp(met),
                                         dp(He), st.ctypes.data_as(C.POINTER(C.c_uint32))))
    return RecoveryEval(met, st, He)


def evaluate_recovery_batch(z, vecH, aod_deg, aoa_deg, tables, *, noise_power, true_idx=None, picks=None, sweep=None,
                            want_H_est=False, out=None, stream=None) -> RecoveryEval:
    """Evaluation_Recovery on device tensors: z [batch][Qt*Qr], vecH [batch][tx*rx] complex128; aod_deg, aoa_deg
    [batch][L] float64; true_idx [batch][L][2] int32 (default: ``tables.true_indices`` in torch); picks [batch][2][2]
    int32 with ``sweep``.  ``out``: a RecoveryEval of an earlier call with the same batch, whose ``metrics`` [batch][15]
    float64, ``status`` [batch] int32 and (with ``want_H_est``) ``H_est`` tensors are reused.  The per-call tables are
    uploaded once per ``tables`` object and device.  Asynchronous on ``stream`` (default: the current stream); nothing
    is copied to the host."""
    import torch
    if not isinstance(tables, RecoveryTables):
        raise TypeError("tables must be a RecoveryTables (recovery_tables(...))")
    ts = [z, vecH, aod_deg, aoa_deg] + [t for t in (true_idx, picks) if t is not None]
    if not all(t.is_cuda for t in ts):
        raise ValueError("evaluate_recovery_batch needs device tensors")
    dev = z.device
    if any(t.device != dev for t in ts):
        raise ValueError("all tensors must be on one device")
    if z.dtype != torch.complex128 or vecH.dtype != torch.complex128:
        raise TypeError("z and vecH must be complex128")
    if aod_deg.dtype != torch.float64 or aoa_deg.dtype != torch.float64:
        raise TypeError("aod_deg and aoa_deg must be float64")
    aod_deg, aoa_deg = aod_deg.contiguous(), aoa_deg.contiguous()
    if true_idx is None:
        if aod_deg.dim() != 2:
            raise ValueError(f"aod_deg must be [batch][L], got {tuple(aod_deg.shape)}")
        true_idx = tables.true_indices(aod_deg, aoa_deg)
    if true_idx.dtype != torch.int32 or (picks is not None and picks.dtype != torch.int32):
        raise TypeError("true_idx and picks must be int32")
    batch, L = _check_shapes(tables, tuple(z.shape), tuple(vecH.shape), tuple(aod_deg.shape), tuple(aoa_deg.shape),
                             tuple(true_idx.shape), None if picks is None else tuple(picks.shape), sweep)
    z, vecH, true_idx = z.contiguous(), vecH.contiguous(), true_idx.contiguous()
    picks = None if picks is None else picks.contiguous()
    nh = tables.tx * tables.rx
    if out is None:
        met = torch.empty((batch, NCOL), dtype=torch.float64, device=dev)
        st = torch.empty(batch, dtype=torch.int32, device=dev)
        He = torch.empty((batch, nh), dtype=torch.complex128, device=dev) if want_H_est else None
    else:
        met, st, He = out.metrics, out.status, out.H_est if want_H_est else None
        if (tuple(met.shape) != (batch, NCOL) or met.dtype != torch.float64 or not met.is_contiguous()
                or tuple(st.shape) != (batch,) or st.dtype != torch.int32 or met.device != dev or st.device != dev):
            raise ValueError(f"out must hold metrics [batch][{NCOL}] float64 and status [batch] int32 on z's device")
        if want_H_est and (He is None or tuple(He.shape) != (batch, nh) or He.dtype != torch.complex128
                           or not He.is_contiguous() or He.device != dev):
            raise ValueError("out.H_est must be [batch][tx*rx] complex128 on z's device")
    up = lambda k: tables._up(k, getattr(tables, k), dev)  # noqa: E731
    A_t, A_r, deg_t, deg_r = up("A_t"), up("A_r"), up("deg_t"), up("deg_r")
    sw, Mt, Mr = [None] * 4, 0, 0
    if sweep is not None:
        names = ("centre_deg_t", "centre_deg_r", "peak_deg_t", "peak_deg_r")
        sw = [torch.from_numpy(np.ascontiguousarray(np.asarray(getattr(sweep, k), np.float64))).to(dev) for k in names]
        Mt, Mr = int(sw[0].shape[0]), int(sw[1].shape[0])
        if int(sw[2].shape[0]) != Mt or int(sw[3].shape[0]) != Mr:
            raise ValueError("sweep: the centre and the peak tables of a side must have one length")
    if stream is None:
        stream = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.ace_evaluate_recovery_batch(batch, tables.tx, tables.rx, L, tables.Qt, tables.Qr, A_t.data_ptr(),
                                          A_r.data_ptr(), deg_t.data_ptr(), deg_r.data_ptr(), tables.first_t,
                                          tables.first_r, _noise(noise_power), tables.kappa, z.data_ptr(), vecH.data_ptr(),
                                          aod_deg.data_ptr(), aoa_deg.data_ptr(), true_idx.data_ptr(), ptr(picks), Mt, Mr,
                                          *[ptr(t) for t in sw], met.data_ptr(), ptr(He), st.data_ptr(),
                                          stream.cuda_stream))
    res = RecoveryEval(met, st, He)
    res._keep = sw   # the sweep tables live until the result does (the launch is asynchronous)
    return res
