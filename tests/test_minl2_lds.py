"""LDS budget of the min-L2 ADMM kernel (CPU test, in the manner of tests/test_gamp_lds.py): minl2_kernel keeps its
state in the caller's workspace and takes no dynamic LDS; its static LDS is the reduction buffer (4 sums x 16 threads
x 32 slots).  This compiles csrc/ace_minl2.hip with the compiler's resource report and checks that static + the
dynamic LDS the launcher requests (ace_lds_request "minl2" at m measurements) fits the CU at m = 1, 130 and 4096 (the
limit), for the loop kernel and for the setup kernels beside it, and that no kernel of the file uses scratch (DESIGN.md
§4h: a conditional between two double2 objects once put a constant on the stack)."""
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "2ace-mmwave-channel-estimation_amd" / "csrc"
HIPCC = "/opt/rocm/bin/hipcc"
LDS_CU = 160 * 1024
_REMARK = re.compile(r"remark: Function Name: (\S+)|remark:\s+LDS Size \[bytes/block\]: (\d+)")
_SCRATCH = re.compile(r"remark: Function Name: (\S+)|remark:\s+ScratchSize \[bytes/lane\]: (\d+)")


@pytest.fixture(scope="module")
def static_lds():
    if not pathlib.Path(HIPCC).exists():
        pytest.skip("hipcc not available")
    cmd = [HIPCC, "--offload-arch=gfx950", "--offload-device-only", "-O3", "-std=c++17",
           "-mllvm", "-amdgpu-mfma-vgpr-form=1", f"-I{ROOT / 'include'}", "-c", str(CSRC / "ace_minl2.hip"),
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
    scratch, name = {}, None
    for m in _SCRATCH.finditer(out.stderr):
        if m.group(1):
            name = m.group(1)
        elif name is not None:
            scratch[name] = int(m.group(2))
            name = None
    res["__scratch__"] = scratch
    return res


def test_no_kernel_of_the_file_uses_scratch(static_lds):
    scratch = static_lds["__scratch__"]
    assert any("minl2_kernel" in k for k in scratch)
    assert all(v == 0 for v in scratch.values()), scratch


@pytest.mark.parametrize("m", [1, 130, 4096])
def test_static_plus_dynamic_fits_the_cu(static_lds, m):
    from ace_amd import _lib
    static_lds = {k: v for k, v in static_lds.items() if k != "__scratch__"}
    hits = {k: v for k, v in static_lds.items() if "minl2_kernel" in k}
    assert len(hits) == 1, sorted(static_lds)
    (kname, static), = hits.items()
    dyn = _lib.lds_request("minl2", m)
    assert dyn == 0
    assert static >= 4 * 16 * 32 * 8   # the reduction buffer
    assert static + dyn <= LDS_CU, f"{kname}: static {static} B + dynamic {dyn} B exceeds {LDS_CU} B"
    for k, v in static_lds.items():   # the setup kernels (the substitution vector of ml_pinv_kernel: 1024 x 16 B)
        assert v <= 64 * 1024, (k, v)


def test_the_launcher_takes_no_lds_attribute():
    text = (CSRC / "ace_minl2.hip").read_text()
    assert "hipFuncSetAttribute" not in text
