"""Angles from a channel matrix, and the exhaustive beam sweep the recovery is measured against.

Host-side numpy around ``scan.beam_scan_*``: the grids and beams are built here, the scan of the channel with
them (``|W^H H F|^2`` over all beam pairs and its strongest entry) runs on the GPU.

The vec(H) order is the synth's (``synth.channel``: element r + rx t), so the leading index is the receive
antenna: combiners go to the scan's ``W0`` (applied conjugated), precoders to ``F1``.  A path with AoD theta_D
and AoA theta_A is ``g a_rx(sin theta_A) a_tx(sin theta_D)^H`` with ``a(s)[k] = exp(-1j kappa s k)``, so the scan
peaks where both steering vectors match.

Noise model.  The reference's sweep measures ``FW vec(H) + W' * noiseMatrix`` (Generate_Measurement.m); the
build's synth draws iid measurement noise CN(0, 10^(-SNR/10)) per probe, and ``beam_sweep`` keeps to the synth's
model: one iid draw per beam pair.
The reference's own model is noise model 1 of ``scenario.scenario_batch`` (``ace_synth_scenario``), on ``kron_codebook``.
"""
from __future__ import annotations

import numpy as np

from . import synth

ST_SWEEP = 8                      # counter-RNG stream kind of the sweep's noise (synth.ST_* are 1..7)
KAPPA = 2.0 * np.pi * (synth.ANT_D / synth.LAMBDA)
SEARCH_DEG = 95.0                 # the synth's angular range (Generate_Channel.m: AoD, AoA ~ U(-47.5, 47.5) deg)


def steering(n_ant, sin_theta, ant_d=None):
    """Array response exp(-1j kappa sin(theta) k) / sqrt(n_ant), k = 0 .. n_ant - 1, one row per entry of
    ``sin_theta`` (Sparse_Channel_Formulation.m:86).  ``ant_d``: the element spacing in metres (kappa = 2 pi ant_d /
    lambda); default the synth's."""
    s = np.atleast_1d(np.asarray(sin_theta, np.float64))
    kappa = KAPPA if ant_d is None else 2.0 * np.pi * (float(ant_d) / synth.LAMBDA)
    ph = kappa * s[:, None] * np.arange(n_ant)[None, :]
    return (np.cos(ph) - 1j * np.sin(ph)) / np.sqrt(n_ant)


def grid_cut(NQ, search_deg=SEARCH_DEG):
    """(sin grid, lo, hi): linspace(-1, 1, NQ + 1)[:-1] (Sparse_Channel_Formulation.m:76-79) and the inclusive
    index range of the grid points nearest sin(-+search_deg / 2) (:114-126, MATLAB's min: the first on a tie)."""
    g = np.linspace(-1.0, 1.0, NQ + 1)[:-1]
    edge = np.sin(np.deg2rad(0.5 * search_deg))
    return g, int(np.argmin(np.abs(g + edge))), int(np.argmin(np.abs(g - edge)))


def dictionary(n_ant, NQ=None, search_deg=SEARCH_DEG, ant_d=None):
    """The steering dictionary of Sparse_Channel_Formulation.m:76-93 with its position-information cut (:114-134):
    (beams [Q][n_ant], their sin grid [Q], their angles in degrees [Q]); NQ = 4 n_ant grid points over sin in
    [-1, 1) by default.  The cut is not optional: at d / lambda = 0.616 the full grid aliases (a steering vector
    at sin theta equals the one at sin theta +- lambda / d), and a peak of the full map may sit on the alias.
    ``ant_d``: the element spacing in metres (default the synth's); ``search_deg = 180`` keeps the whole grid, which
    is what the directional driver's Searching_Area = 180 does."""
    NQ = 4 * n_ant if NQ is None else int(NQ)
    g, lo, hi = grid_cut(NQ, search_deg)
    s = g[lo:hi + 1]
    return steering(n_ant, s, ant_d), s, np.rad2deg(np.arcsin(s))


_J = np.array([-1.0, -1j, 1.0, 1j, -1.0])   # exp(1j phi) on -pi : pi/2 : pi, exactly


def quantize_ps(v, bits=2):
    """Quantize_PS.m:61-72 without its 1 / sqrt(rows): each entry's phase to the nearest of -pi : 2 pi / 2^bits : pi,
    a tie to the smaller angle (``min`` takes the first), unit modulus.  At 2 bits the values are exact powers of j."""
    v = np.asarray(v, np.complex128)
    nps = 2 ** int(bits)
    phi = -np.pi + (2.0 * np.pi / nps) * np.arange(nps + 1)
    ind = np.argmin(np.abs(np.angle(v)[..., None] - phi), axis=-1)
    return _J[ind] if nps == 4 else np.cos(phi[ind]) + 1j * np.sin(phi[ind])


def sweep_beams(n_ant, M, search_deg=SEARCH_DEG):
    """MyBeamSweeping.m:93-108: (beams [M][n_ant], centre angles in degrees [M]) -- the steering vectors at the
    centres of M equal partitions of [-search_deg / 2, search_deg / 2], quantised to 2 bits (unit modulus)."""
    part = np.linspace(-0.5 * search_deg, 0.5 * search_deg, int(M) + 1)
    centres = 0.5 * (part[:-1] + part[1:])
    return quantize_ps(steering(n_ant, np.sin(np.deg2rad(centres))) * np.sqrt(n_ant)), centres


def directional_beams(n_ant, M, search_deg=SEARCH_DEG):
    """Directional_Beam_Angular.m:72-85 for one side: (beams [M][n_ant], centre angles in degrees [M]).  An alias of
    ``sweep_beams``: the reference builds pattern 1's probes (Directional_Beam_Angular.m:79-85, steering vectors over
    sqrt(N)) and pattern 2's sweep beams (MyBeamSweeping.m:101-108, unnormalised) at the same partition centres, and
    Quantize_PS keeps only the phases, so the two give the same F and W.  Unit modulus here; the reference's beams are
    these over sqrt(n_ant) (Quantize_PS.m:70)."""
    return sweep_beams(n_ant, M, search_deg)


def peak_angle_grid():
    """The 36001 angles -90 : 0.005 : 90 of MyBeamSweeping.m:134, built from both ends as MATLAB's colon does."""
    i = np.arange(36001)
    return np.where(i <= 18000, -90.0 + 0.005 * i, 90.0 - 0.005 * (36000 - i))


def beam_peak_angles(beams):
    """Pattern 1's angle estimate (MyBeamSweeping.m:134-154) on the GPU (``ace_beam_peak_angles``): for each beam
    [M][n_ant] the first angle of ``peak_angle_grid()`` that maximises |f^H a(theta)|, a the unnormalised steering
    vector; degrees [M].  Once per sweep point.  A numpy array in gives a numpy array; a device tensor a device tensor."""
    import ctypes as C
    from ._lib import LIB, check
    if isinstance(beams, np.ndarray) or not hasattr(beams, "is_cuda"):
        b = np.ascontiguousarray(np.atleast_2d(np.asarray(beams, np.complex128)))
        if b.ndim != 2 or not 1 <= b.shape[1] <= 32 or b.shape[0] < 1:
            raise ValueError(f"beams must be [M][n_ant] with 1 <= n_ant <= 32, got {b.shape}")
        out = np.empty(b.shape[0], np.float64)
        dp = lambda a: a.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        check(LIB.ace_beam_peak_angles_host(b.shape[0], b.shape[1], float(KAPPA), dp(b), dp(out)))
        return out
    import torch
    if not beams.is_cuda or beams.dtype != torch.complex128 or beams.dim() != 2 or not 1 <= beams.shape[1] <= 32:
        raise ValueError("beams must be a complex128 device tensor [M][n_ant] with 1 <= n_ant <= 32")
    b = beams.contiguous()
    out = torch.empty(b.shape[0], dtype=torch.float64, device=b.device)
    check(LIB.ace_beam_peak_angles(int(b.shape[0]), int(b.shape[1]), float(KAPPA), b.data_ptr(), out.data_ptr(),
                                   torch.cuda.current_stream(b.device).cuda_stream))
    return out


def kron_codebook(Ft, Wr):
    """The measurement matrix kron(F.', W') of Generate_Sensing_Matrix.m for precoders Ft [Mt][tx] and combiners Wr
    [Mr][rx] given as rows: A [Mt*Mr][tx*rx] with A[it Mr + q][t rx + r] = Ft[it][t] conj(Wr[q][r]), the synth's vec(H)
    order (element r + rx t), so (A vecH)[it Mr + q] = w_q^H H f_it.  ``sweep_beams`` is Directional_Beam_Angular.m's
    beam set (the steering vectors at the centres of M equal partitions of the searching area, quantised to 2 bits);
    the reference's 'Directional_Beam_Angular' codebook is ``kron_codebook(sweep_beams(tx, Mt, deg)[0] / sqrt(tx),
    sweep_beams(rx, Mr, deg)[0] / sqrt(rx))``."""
    Ft, Wr = np.atleast_2d(np.asarray(Ft, np.complex128)), np.atleast_2d(np.asarray(Wr, np.complex128))
    A = Ft[:, None, :, None] * np.conj(Wr)[None, :, None, :]           # [it][q][t][r]
    return np.ascontiguousarray(A.reshape(Ft.shape[0] * Wr.shape[0], Ft.shape[1] * Wr.shape[1]))


def _scan(X, W0, F1, noise=None, **kw):
    """beam_scan_batch for device tensors (beams and noise uploaded), beam_scan_host for numpy arrays."""
    from .scan import beam_scan_batch, beam_scan_host
    if isinstance(X, np.ndarray):
        return beam_scan_host(X, W0, F1, 1, noise, **kw), (lambda a: np.asarray(a))
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(X.device)  # noqa: E731
    return beam_scan_batch(X, up(W0), up(F1), 1, up(noise), **kw), up


def estimate_angles(X, tx, rx, NQ_t=None, NQ_r=None, search_deg=SEARCH_DEG):
    """The strongest entry of the angular map A_Rx' * mat(x) * A_Tx (Sparse_Channel_Formulation.m:149) over the
    two cut dictionaries, as Evaluation_Recovery.m:101-113 reads an angle off a grid index: (aod_deg, aoa_deg,
    power, p, q) per realisation, p / q the indices into ``dictionary(tx)`` / ``dictionary(rx)``.  X [batch][tx*rx]
    in the synth's vec(H) order: a device tensor (the results are device tensors) or a numpy array."""
    Ft, _, deg_t = dictionary(tx, NQ_t, search_deg)
    Wr, _, deg_r = dictionary(rx, NQ_r, search_deg)
    res, up = _scan(X, Wr, Ft)
    p, q = res.p[:, 0], res.q[:, 0]
    pl, ql = (p.astype(np.int64), q.astype(np.int64)) if isinstance(p, np.ndarray) else (p.long(), q.long())
    # (a degenerate realisation has p = q = -1: the last grid point, flagged by res.status)
    return up(deg_t)[pl], up(deg_r)[ql], res.top_pow[:, 0], p, q


def sweep_noise(seed, first, count, Mt, Mr, snr_db):
    """The sweep's noise [count][Mt*Mr]: CN(0, 10^(-snr_db / 10)) per beam pair from the counter RNG, stream kind
    ST_SWEEP of realisation first + b, counter = the flat pair index p Mr + q."""
    sig = np.sqrt(0.5 * 10.0 ** (-snr_db / 10.0))
    return np.stack([synth.normal_pairs(seed, synth.stream_id(ST_SWEEP, first + b), Mt * Mr) * sig
                     for b in range(count)])


def beam_sweep(H, tx, rx, Mt, Mr, *, snr_db, seed, first=0, search_deg=SEARCH_DEG):
    """The exhaustive sweep of MyBeamSweeping.m (pattern 2): Mt x Mr quantised directional beams scaled by
    1 / sqrt(tx rx) like the synth's codebook rows (:107-109), RSS = |FW vec(H) + noise|^2, the strongest pair
    (:119-125) and its centre angles (:156-157): (aod_deg, aoa_deg, p, q) per realisation.  H [batch][tx*rx] is
    the channel at the synth's scale (``synth.channel``), realisation b of the call being realisation first + b
    of the sweep: its noise depends on (seed, first + b) alone."""
    Ft, cen_t = sweep_beams(tx, Mt, search_deg)
    Wr, cen_r = sweep_beams(rx, Mr, search_deg)
    noise = sweep_noise(seed, first, int(H.shape[0]), Mt, Mr, snr_db)
    res, up = _scan(H, Wr / np.sqrt(rx), Ft / np.sqrt(tx), noise)
    p, q = res.p[:, 0], res.q[:, 0]
    pl, ql = (p.astype(np.int64), q.astype(np.int64)) if isinstance(p, np.ndarray) else (p.long(), q.long())
    return up(cen_t)[pl], up(cen_r)[ql], p, q


def aoda_err(aod, aoa, aod_true, aoa_true):
    """(|dAoD| + |dAoA|) / 2 against the nearest true path (Evaluation_Recovery.m:135-146 for the one estimated
    path: the minimum over the L true ones), degrees.  aod, aoa [batch]; aod_true, aoa_true [batch][L]."""
    e = 0.5 * (np.abs(np.asarray(aod)[:, None] - aod_true) + np.abs(np.asarray(aoa)[:, None] - aoa_true))
    return e.min(axis=1)
