"""Resource table of every kernel in csrc/*.hip: the compiler's gfx950 resource report (the compile
and parser of tests/test_lds_budget.py), reduced to registers, spills, scratch, LDS and occupancy.

    python tools/kernel_resources.py table <out.json> [checkout root]
    python tools/kernel_resources.py compare <parent.json> <branch.json> <merged.json>

`compare` writes {"parent": ..., "branch": ..., "violations": [...]} and fails unless, for every
kernel, LDS is equal, occupancy is not lower, and scratch and spilled VGPRs are not higher."""
import concurrent.futures as cf
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from test_lds_budget import CSRC, _resources   # noqa: E402

KEEP = {"VGPRs": "vgprs", "AGPRs": "agprs", "TotalSGPRs": "sgprs", "VGPRs Spill": "vgprs_spilled",
        "ScratchSize": "scratch_bytes", "LDS Size": "lds_bytes", "Occupancy": "occupancy"}


def table(root):
    srcs = sorted(p.name for p in (pathlib.Path(root) / CSRC.relative_to(ROOT)).glob("*.hip"))
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        reports = ex.map(lambda s: _resources(s, root), srcs)
    return {src: {k: {KEEP[f]: v[f] for f in KEEP} for k, v in sorted(rep.items())}
            for src, rep in zip(srcs, reports)}


def violations(parent, branch):
    bad = []
    for src in sorted(set(parent) | set(branch)):
        p, b = parent.get(src, {}), branch.get(src, {})
        for k in sorted(set(p) | set(b)):
            if k not in p or k not in b:
                bad.append(f"{src}: {k} only in the {'parent' if k in p else 'branch'}")
                continue
            for f, worse in (("lds_bytes", p[k]["lds_bytes"] != b[k]["lds_bytes"]),
                             ("occupancy", b[k]["occupancy"] < p[k]["occupancy"]),
                             ("scratch_bytes", b[k]["scratch_bytes"] > p[k]["scratch_bytes"]),
                             ("vgprs_spilled", b[k]["vgprs_spilled"] > p[k]["vgprs_spilled"])):
                if worse:
                    bad.append(f"{src}: {k}: {f} {p[k][f]} -> {b[k][f]}")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "table":
        t = table(sys.argv[3] if len(sys.argv) > 3 else ROOT)
        pathlib.Path(sys.argv[2]).write_text(json.dumps(t, indent=1) + "\n")
        print(f"{sum(len(v) for v in t.values())} kernels in {len(t)} sources")
    else:
        parent, branch = (json.loads(pathlib.Path(a).read_text()) for a in sys.argv[2:4])
        bad = violations(parent, branch)
        pathlib.Path(sys.argv[4]).write_text(
            json.dumps({"parent": parent, "branch": branch, "violations": bad}, indent=1) + "\n")
        print("\n".join(bad) or "no kernel is worse than the parent's")
        sys.exit(1 if bad else 0)
