"""Does the operator setup run beside init?  Per solve of a rocprofv3 kernel trace of the unit bench
(`bench.py --steps K`): the span and device time of the setup kernels and their streams, the span of the
init Z-step, the overlap of the two, and the time from the solve's first setup / init kernel to its
first iteration launch.  Diagnostic only.
usage: setup_overlap.py run_kernel_trace.csv"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
K = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r["Stream_Id"]) for r in rows)
SETUP = ("zgemm3m_kernel<0, false", "zgemm3m_kernel<1, true", "zgemm3m_kernel<2, true", "hermitize", "ns_prep", "max_abs",
         "i8_expand", "i8k_expand", "conj_transpose", "gyk_gfrag")
def is_setup(n): return any(k in n for k in SETUP)
inits = [i for i, k in enumerate(K) if "zstep1w_kernel<true>" in k[2]]
print(f"{len(K)} kernels, {len(inits)} solves")
for si, i in enumerate(inits):
    zs, ze = K[i][0], K[i][1]
    # setup kernels of this solve: those within 3 ms before / during the init Z-step
    st = [k for k in K if is_setup(k[2]) and zs - 3_000_000 < k[0] < ze + 3_000_000]
    first_it = next((k for k in K[i:] if "gyf_kernel" in k[2] or "gyk_kernel" in k[2]), None)
    if not st or not first_it: continue
    s0, s1 = min(k[0] for k in st), max(k[1] for k in st)
    begin = min(s0, min(k[0] for k in K if zs - 3_000_000 < k[0] and ("init_r" in k[2] or is_setup(k[2]))))
    ov = max(0, min(s1, ze) - max(s0, zs))
    print(f"solve {si}: setup span {(s1 - s0) / 1e3:7.1f} us ({len(st)} kernels, device {sum(k[1]-k[0] for k in st)/1e3:6.1f} us, streams {sorted(set(k[3] for k in st))}), "
          f"init Z-step {(ze - zs) / 1e3:6.1f} us (stream {K[i][3]}), overlap {ov / 1e3:6.1f} us, "
          f"first setup/init kernel -> first iteration launch {(first_it[0] - begin) / 1e3:7.1f} us")
