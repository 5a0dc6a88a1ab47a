"""GPU test of pattern 1's angle estimate (ace_beam_peak_angles: MyBeamSweeping.m:134-154) against the numpy
restatement tests/recovery_ref.py::peak_angles on the quantised directional beams.

The restatement's gain at the returned angle must lie within 1e-12 sqrt(N) of the restatement's maximum (the gain
is a sum of N unit-modulus terms; the two evaluations of it differ by rounding); where no angle other than the
restatement's pick lies inside that band, the angle must be the restatement's."""
import pathlib
import sys

import numpy as np
import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import recovery_ref as RR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("M", [2, 8])
@pytest.mark.parametrize("N", [1, 4, 12, 16, 32])
def test_peak_angles_of_the_directional_beams(gpu, N, M):
    import torch
    from ace_amd import angular
    beams, centres = angular.directional_beams(N, M, 95.0)
    grid = angular.peak_angle_grid()
    ref, gain = RR.peak_angles(beams, angular.KAPPA, grid)
    got = angular.beam_peak_angles(beams)
    dev = angular.beam_peak_angles(torch.from_numpy(beams).to(gpu)).cpu().numpy()
    assert got.shape == (M,) and np.array_equal(got, dev)
    band = 1e-12 * np.sqrt(N)
    for m in range(M):
        i = np.flatnonzero(grid == got[m])
        assert len(i) == 1, (m, got[m])          # an angle of the grid itself
        assert gain[m, i[0]] >= gain[m].max() - band, (m, got[m], ref[m])
        inside = np.flatnonzero(gain[m] >= gain[m].max() - band)
        if len(inside) == 1:
            assert got[m] == ref[m], (m, got[m], ref[m])
        else:
            assert i[0] >= inside[0], (m, got[m])   # never before the first angle of the band
    if N == 1:
        assert (got == -90.0).all()              # a single antenna has a flat pattern: the first angle wins
