"""LDS budget of the beam scan kernel (CPU test, in the manner of tests/test_lds_budget.py): scan_kernel takes
84480 B of dynamic LDS, past the 64 KiB default, through its derived budget (lds_dyn_budget: the CU's 160 KiB less
the kernel's static LDS).  This compiles csrc/ace_scan.hip with the compiler's resource report and checks, for
each of the three list sizes the launcher instantiates (K = 1, K <= 4, K <= 16), that static + the dynamic LDS the
launcher requests (ace_lds_request "scan") fits the CU.  The request is the same at every shape (the tiles are
fixed: mat(x) 32 x 32, a 64-row T tile, a 64-row beam tile), so the shapes of tests/scan_ref.py are all covered by
one number; the test states that too."""
import pathlib
import re
import subprocess
import sys

import pytest

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import scan_ref as SR  # noqa: E402

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
           "-mllvm", "-amdgpu-mfma-vgpr-form=1", f"-I{ROOT / 'include'}", "-c", str(CSRC / "ace_scan.hip"),
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


@pytest.mark.parametrize("kc", [1, 4, 16])
def test_static_plus_dynamic_fits_the_cu(static_lds, kc):
    from ace_amd import _lib
    hits = {k: v for k, v in static_lds.items() if re.search(rf"scan_kernelILi{kc}E", k)}
    assert len(hits) == 1, sorted(static_lds)
    (kname, static), = hits.items()
    requests = {_lib.lds_request("scan", max(d0, d1, Q0, Q1)) for _, d0, d1, Q0, Q1, _ in SR.SHAPES}
    assert len(requests) == 1            # the same at every tested shape
    (dyn,) = requests
    assert dyn == (32 + 64 + 64) * 33 * 16
    assert 64 * 1024 < dyn and static + dyn <= LDS_CU, f"{kname}: static {static} B + dynamic {dyn} B exceeds {LDS_CU} B"


def test_the_launcher_goes_through_the_derived_budget():
    text = (CSRC / "ace_scan.hip").read_text()
    assert "lds_ok(" in text and "hipFuncSetAttribute" not in text
