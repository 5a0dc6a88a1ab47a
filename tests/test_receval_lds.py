"""LDS budget of the recovery evaluator's kernel (CPU test, in the manner of tests/test_omp_lds.py): receval_kernel
takes up to 95232 B of dynamic LDS (the SVD workspace of the channel evaluator, H_est, H and the 16-column tile of
A_r^T mat(z)^T), past the 64 KiB default, through its derived budget (lds_dyn_budget: the CU's 160 KiB less the
kernel's static LDS).  This compiles csrc/ace_receval.hip with the compiler's resource report and checks that static +
the dynamic LDS the launcher requests (ace_lds_request "receval" / "receval_rect" at N = max(tx, rx)) fits the CU, and
that mat(z) itself is nowhere in it."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "2ace-mmwave-channel-estimation_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
LDS_CU = 160 * 1024
_REMARK = re.compile(r"remark: Function Name: (\S+)|remark:\s+LDS Size \[bytes/block\]: (\d+)")


@pytest.fixture(scope="module")
def static_lds():
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17",
           "-mllvm", "-amdgpu-mfma-vgpr-form=1", f"-I{ROOT / 'include'}", "-c", str(CSRC / "ace_receval.hip"),
           "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for m in _REMARK.finditer(out.stderr):
        if m.group(1):
            name = m.group(1)
        elif name is not None:
            res[name] = int(m.group(2))
            name = None
    return res


def _expected(N, rect):
    nt = (N + 15) // 16
    return (3 if rect else 2) * N * (N + 1) * 16 + 5 * 32 * 16 + 2 * 32 * 8 + 2 * N * N * 16 + nt * 16 * 17 * 16


@pytest.mark.parametrize("rect", [False, True])
@pytest.mark.parametrize("N", [1, 4, 12, 16, 17, 32])
def test_static_plus_dynamic_fits_the_cu(static_lds, N, rect):
    from ace_amd import _lib
    hits = {k: v for k, v in static_lds.items() if "receval_kernel" in k}
    assert len(hits) == 4, sorted(static_lds)   # square / rectangular x one / two 16-row tiles
    dyn = _lib.lds_request("receval_rect" if rect else "receval", N)
    assert dyn == _expected(N, rect)
    for kname, static in hits.items():
        assert static <= 1024, (kname, static)
        assert static + dyn <= LDS_CU, f"{kname}: static {static} B + dynamic {dyn} B exceeds {LDS_CU} B"
    if N == 32:
        assert dyn == (95232 if rect else 78336) and dyn > 64 * 1024
        assert dyn < 128 * 128 * 16   # mat(z) at Qt = Qr = 128 alone is 256 KiB: it is tiled, not held


def test_the_launcher_goes_through_the_derived_budget():
    text = (CSRC / "ace_receval.hip").read_text()
    assert "lds_ok(" in text and "hipFuncSetAttribute" not in text
    peak = [k for k in ("peak_kernel",) if k in text]
    assert peak
