"""Drop-in for the MATLAB Engine session main.py drives (main/main.py:10, :308, :427-437).

The reference calls, e.g.::

    eng = matlab.engine.start_matlab()
    H_amp, H_angle = eng.channel_recovery_ADMM_v2_simulation_A2only(
        int(num_ant), int(num_ant), matlab.double(np.abs(cb).tolist()),
        matlab.double(np.angle(cb).tolist()), matlab.double(rss.tolist()), eng.double(r+1), nargout=2)
    H = np.squeeze(np.array(H_amp) * np.exp(1j * np.array(H_angle)))       # 8 x n

With this module::

    from ace_amd import engine as matlab_engine
    eng = matlab_engine.start_matlab()
    H_amp, H_angle = eng.channel_recovery_ADMM_v2_simulation_A2only(..., nargout=2)

accepts the same arguments (``matlab.double`` lists, numpy arrays, ``eng.double``
scalars), returns numpy arrays of MATLAB's shape (n_M, 1, n) -- (n_M, 2, n) for the directional driver of
main.py:231, whose two methods are PLOMP and PLGAMP (``recover_directional``) -- and raises
``MatlabExecutionError`` where the MATLAB function calls ``error``.  Each call runs
the full recovery pipeline per sweep point on the GPU through
``ace_recover_driver`` (libace.so); nothing falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import LIB, AceError, ACE_ERR_ARG

DRIVER_A2ONLY, DRIVER_A2NUCLEAR, DRIVER_MULTIRES, DRIVER_PHASELIFT = 0, 1, 2, 3
RSS_FCT = 1e5 / 3  # channel_recovery_ADMM_v2_simulation_A2only.m:125


class MatlabExecutionError(RuntimeError):
    """Raised where the reference MATLAB function raises (error(...))."""


def double(x):
    """matlab.double / eng.double stand-in: a float64 numpy array (or scalar)."""
    a = np.asarray(x, dtype=np.float64)
    return a if a.ndim else float(a)


LIB.ace_recover_driver.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                   C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double)]
LIB.ace_recover_driver.restype = C.c_int
LIB.ace_recover_driver_ex.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.c_int,
                                      C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
LIB.ace_recover_driver_ex.restype = C.c_int
LIB.ace_driver_m_sweep.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int32)]
LIB.ace_driver_m_sweep.restype = C.c_int
LIB.ace_driver_randperm.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_int32)]
LIB.ace_driver_randperm.restype = C.c_int


def m_sweep(tx, rx):
    """The reference's 8-point M sweep (..._A2only.m:106-118)."""
    out = (C.c_int32 * 8)()
    k = LIB.ace_driver_m_sweep(int(tx), int(rx), out)
    if k < 0:
        raise MatlabExecutionError(LIB.ace_last_error().decode())
    return np.array(out[:k], dtype=np.int64)


def randperm(seed, stream, P, k):
    """randperm(P, k) (0-based) from the build's counter RNG."""
    out = np.empty(k, np.int32)
    rc = LIB.ace_driver_randperm(int(seed), int(stream), int(P), int(k), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc < 0:
        raise ValueError(LIB.ace_last_error().decode())
    return out


def recover(driver, tx_ant_num, rx_ant_num, cb_amp, cb_angle, rss_final, seed_id, M_list=None, maxiter=0):
    """ace_recover_driver on numpy inputs; returns (H_amp, H_angle) of shape (n_M, 1, n).  ``maxiter`` > 0
    caps every solve's iterations (ace_recover_driver_ex; parity runs on a stable horizon)."""
    tx, rx = int(tx_ant_num), int(rx_ant_num)
    amp = np.ascontiguousarray(np.asarray(cb_amp, dtype=np.float64))
    ang = np.ascontiguousarray(np.asarray(cb_angle, dtype=np.float64))
    rss = np.ascontiguousarray(np.asarray(rss_final, dtype=np.float64).reshape(-1))
    n = tx * rx
    if amp.ndim != 2 or amp.shape != ang.shape or amp.shape[1] != n or rss.size != amp.shape[0]:
        raise MatlabExecutionError(f"codebook/rss shapes {amp.shape}/{ang.shape}/{rss.shape} do not match "
                                   f"{tx}x{rx} antennas")
    P = amp.shape[0]
    if M_list is None:
        Ms = None
        nM = 8
    else:
        Ms = np.ascontiguousarray(np.asarray(M_list, dtype=np.int32).reshape(-1))
        nM = Ms.size
    H_amp = np.zeros((nM, n), np.float64)
    H_ang = np.zeros((nM, n), np.float64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = LIB.ace_recover_driver_ex(int(driver), tx, rx, P, dp(amp), dp(ang), dp(rss), int(seed_id), int(nM),
                                   None if Ms is None else Ms.ctypes.data_as(C.POINTER(C.c_int32)), int(maxiter),
                                   dp(H_amp), dp(H_ang))
    if rc < 0:
        msg = LIB.ace_last_error().decode()
        if rc == ACE_ERR_ARG and "unknown driver" not in msg:
            raise MatlabExecutionError(msg)
        raise AceError(rc, msg)
    return H_amp[:rc, None, :], H_ang[:rc, None, :]


def _mround(x):
    """MATLAB's round (halves away from zero) for positive arguments."""
    return np.floor(np.asarray(x, np.float64) + 0.5).astype(np.int64)


DIRECTIONAL_ANT_D = 2.9e-3   # channel_recovery_ADMM_v2_simulation_directional.m:41 (the other drivers: 3.055e-3)
DIRECTIONAL_GRID = 32        # the directional codebook is 32 x 32 beam pairs


def directional_sweep(tx, rx):
    """Mt of channel_recovery_ADMM_v2_simulation_directional.m:105-126: round(linspace(2, sqrt(4 tx rx), 8)), with
    tx - 1, rx - 1 at 17 antennas; the function calls error() for other antenna counts (and leaves Mt undefined at 4)."""
    tx, rx = int(tx), int(rx)
    if 8 in (tx, rx) or 16 in (tx, rx) or 32 in (tx, rx) or 36 in (tx, rx):
        top = np.sqrt(4.0 * tx * rx)
    elif 17 in (tx, rx):
        top = np.sqrt(4.0 * (tx - 1) * (rx - 1))
    elif 4 in (tx, rx):
        raise MatlabExecutionError("Undefined function or variable 'Mt'.")
    else:
        raise MatlabExecutionError("Number of antenna on Tx and Rx must be 4/8/16/32!")
    return _mround(np.linspace(2.0, top, 8))


def recover_directional(tx_ant_num, rx_ant_num, cb_amp, cb_angle, rss_final, seed_id, Mt_list=None, pl_maxits=4000,
                        device=None):
    """channel_recovery_ADMM_v2_simulation_directional.m: the two-stage recoveries PLOMP (slot 0) and PLGAMP (slot 1)
    from the RSS of the directional codebook.  cb_amp, cb_angle: 32 x 32 x n (n = tx rx); rss_final: 32 x 32 dBm.
    Per sweep point M of ``Mt_list`` (default ``directional_sweep``): indexing = round(linspace(1, 32, min(M, 32))),
    beams = reshape(cb(indexing, indexing, :), [M^2, n]) in MATLAB's column-major order, measurements =
    sqrt(db2pow(rss) / 1000) 1e5/3, then the PLOMP / PLGAMP branch of Recover_Channel.m:38-44:
    My_TwoStage_Recovery((meas / 2e5)^2 1e10, beams AD, s = 3, noise_power = 1) on the dictionary AD of this driver's
    own ULA (d = 2.9 mm, NQ = 4 antennas per side, Searching_Area = 180: the whole grid), H = AD signal / sqrt(1e10)
    2e5 / rss_fct, NaN -> 0.  Returns (|H|, angle(H)), each (len(Mt_list), 2, n).  ``seed_id`` is accepted and, as in
    the reference (whose only random draw, Generate_Channel, does not reach the output), not used.

    The reference's own reshape fails for a sweep point with M > 32 (cb_train has 32^2 rows, not M^2): MATLAB stops
    there with an error, and so does this function, with a ValueError naming the point.  That is every full sweep
    at 32 antennas and above."""
    import torch
    from . import sparse
    tx, rx = int(tx_ant_num), int(rx_ant_num)
    n = tx * rx
    G = DIRECTIONAL_GRID
    amp = np.asarray(cb_amp, dtype=np.float64)
    ang = np.asarray(cb_angle, dtype=np.float64)
    rss = np.asarray(rss_final, dtype=np.float64)
    if amp.shape != (G, G, n) or ang.shape != amp.shape or rss.shape != (G, G):
        raise MatlabExecutionError(f"codebook/rss shapes {amp.shape}/{ang.shape}/{rss.shape} do not match "
                                   f"{G} x {G} x {n} and {G} x {G}")
    Ms = directional_sweep(tx, rx) if Mt_list is None else np.asarray(Mt_list, np.int64).reshape(-1)
    cb = amp * np.exp(1j * ang)
    dev = torch.device("cuda" if device is None else device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    AD = up(sparse.dictionary_2d(tx, rx, 4 * tx, 4 * rx, 180.0, DIRECTIONAL_ANT_D)[0])
    H = np.zeros((len(Ms), 2, n), np.complex128)
    for i, M in enumerate(int(m) for m in Ms):
        if M < 1:
            raise ValueError(f"sweep point {i}: M = {M} < 1")
        if M > G:
            raise ValueError(f"sweep point {i}: M = {M} > {G}: the reference's reshape(cb_train, [M^2, n]) fails there "
                             f"(cb_train holds {G}^2 beam pairs), and MATLAB stops with an error")
        idx = _mround(np.linspace(1.0, float(G), M)) - 1
        beams = cb[np.ix_(idx, idx)].transpose(1, 0, 2).reshape(M * M, n)        # row i + M j (column-major)
        rss_train = rss[np.ix_(idx, idx)].T.reshape(M * M)
        meas = np.sqrt(10.0 ** (rss_train / 10.0) / 1000.0) * RSS_FCT
        meas_sq = (meas / 2e5) ** 2 * 1e10
        Phi = (up(beams) @ AD).contiguous()
        omp, gamp = sparse.two_stage_batch(Phi, up(meas_sq[None, :]), 3, 1.0, maxIts=int(pl_maxits))
        for slot, r in enumerate((omp, gamp)):
            H[i, slot] = r.channel(AD)[0].cpu().numpy() / np.sqrt(1e10) * 2e5 / RSS_FCT
    H[np.isnan(H)] = 0
    return np.abs(H), np.angle(H)


class Engine:
    """Object with the MATLAB function names main.py calls on its engine."""

    @staticmethod
    def double(x):
        return double(x)

    def _call(self, driver, args, nargout):
        """One path for all five drivers: the nargout check here, the conversion of the Engine's argument types
        (``matlab.double`` lists, numpy arrays, ``eng.double`` scalars -> float64 arrays, ints) in ``recover`` /
        ``recover_directional``, which both take the MATLAB argument list as it is."""
        if nargout != 2:
            raise MatlabExecutionError("these functions return [H_amp, H_angle] (nargout=2)")
        if callable(driver):
            return driver(*args)
        return recover(driver, *args)

    def channel_recovery_ADMM_v2_simulation_A2only(self, *args, nargout=2):
        return self._call(DRIVER_A2ONLY, args, nargout)

    def channel_recovery_ADMM_v2_simulation_A2nuclear(self, *args, nargout=2):
        return self._call(DRIVER_A2NUCLEAR, args, nargout)

    def channel_recovery_ADMM_v2_simulation_multiresolution(self, *args, nargout=2):
        return self._call(DRIVER_MULTIRES, args, nargout)

    def channel_recovery_ADMM_v2_simulation_phaselift(self, *args, nargout=2):
        return self._call(DRIVER_PHASELIFT, args, nargout)

    def channel_recovery_ADMM_v2_simulation_directional(self, *args, nargout=2):
        """main.py:231, the first estimator call of the script: (H_amp, H_angle), each 8 x 2 x n (PLOMP, PLGAMP)."""
        return self._call(recover_directional, args, nargout)

    def quit(self):
        pass


def start_matlab(*_args, **_kw):
    """matlab.engine.start_matlab() stand-in."""
    return Engine()
