// Test entries for the four linear operators of the ADMM iteration (ace_linop_host) and for the f64
// 3M GEMM launcher (ace_zgemm_host): host arrays in, one operator application, host arrays out.
//
// Nothing is re-implemented here.  The operators are carved and built by linops_carve /
// linops_setup exactly as a solve builds them, the per-realisation control blocks are filled from
// the caller's mu / vbound / done / nzero / avok (every other field zero), and each operator makes
// the launcher calls admm_run makes for it on the chosen path (ace_admm.cpp: applyA / applyMM /
// applyAH, the fused and int8 branches of the iteration).  The fused kernels whose control state
// is the solver's (gyk / gyf / msr, the FUSE epilogue of i8ah_kernel) have an entry of their own
// (ace_unit_host, ace_unit_host.cpp), as have pgk and the private code-image setup (ace_pc_host,
// ace_pc_host.cpp).
#include "ace_host.hpp"

namespace ace {
namespace {

int linop_run(const ace_linop_args& a) {
    const int m = a.m, n = a.n, batch = a.batch, r = a.rcols, op = a.op, path = a.path;
    const bool shared = a.a_shared != 0, i8 = path == ACE_LINOP_I8;
    if (op < ACE_LINOP_A || op > ACE_LINOP_SETUP || path < ACE_LINOP_F64 || path > ACE_LINOP_I8)
        return fail(ACE_ERR_ARG, "ace_linop_host: unknown op %d / path %d", op, path);
    if (m < 1 || n < 1 || batch < 1 || r < 1 || m > 4096 || n > 4096 || (long long)batch * r > (1 << 20))
        return fail(ACE_ERR_ARG, "ace_linop_host: bad shape (m %d, n %d, batch %d, rcols %d)", m, n, batch, r);
    if (!a.A || !a.out || !a.mu) return fail(ACE_ERR_ARG, "ace_linop_host: NULL A / out / mu");
    if (!shared && (r != 1 || path != ACE_LINOP_F64))
        return fail(ACE_ERR_UNSUPPORTED, "ace_linop_host: private codebooks run the f64 GEMV path at rcols = 1");
    if (path == ACE_LINOP_F64_FUSED && (r != 1 || (op != ACE_LINOP_A && op != ACE_LINOP_AH)))
        return fail(ACE_ERR_UNSUPPORTED, "ace_linop_host: the fused f64 GEMMs are apply_A / apply_AH at rcols = 1");
    if (i8 && op == ACE_LINOP_G) return fail(ACE_ERR_UNSUPPORTED, "ace_linop_host: g = G T has no int8 form");
    if (a.AX && !(i8 && op == ACE_LINOP_A && r == 1))
        return fail(ACE_ERR_ARG, "ace_linop_host: AX belongs to the int8 apply_A at rcols = 1");
    const bool needZ = op == ACE_LINOP_A || (op == ACE_LINOP_AH && !(i8 && r == 1));
    const bool needY = op == ACE_LINOP_A;
    const bool needg = op == ACE_LINOP_AH || op == ACE_LINOP_K || op == ACE_LINOP_G;
    if ((needZ && !a.Z) || (needY && !a.Y) || (needg && !a.g)) return fail(ACE_ERR_ARG, "ace_linop_host: NULL operand");
    if (op == ACE_LINOP_SETUP && !a.out2) return fail(ACE_ERR_ARG, "ace_linop_host: setup needs out2 (G)");

    const int nv = batch * r, mats = shared ? 1 : batch;
    const size_t bn = 2 * (size_t)nv * n, bm = 2 * (size_t)nv * m;   // doubles of an n- / m-space operand
    const long long mm = (long long)m * m, mn = (long long)m * n;

    // one allocation: the operators, then this entry's operands
    LinOps L;
    double *dA, *dZ, *dN, *dY, *dM, *dV, *dS, *dg, *dAX, *dout, *dzeros;
    RealState* drs;
    auto carve = [&](Carver& cv) {
        linops_carve(cv, shared, batch, m, n, &L);
        dA = cv.take(16 * (size_t)mats * mn);
        dZ = cv.take(8 * bn);
        dN = cv.take(8 * bn);
        dV = cv.take(8 * bn);
        dY = cv.take(8 * bm);
        dM = cv.take(8 * bm);
        dS = cv.take(8 * bm);
        dg = cv.take(8 * bm);
        dAX = cv.take(8 * bm);
        dout = cv.take(8 * (bn > bm ? bn : bm));
        dzeros = cv.take(16 * (size_t)n);
        drs = cv.take<RealState>(sizeof(RealState) * (size_t)batch);
    };
    DevScope d;
    ACE_TRY(carve_zeroed(d, carve));
    hipStream_t st = nullptr;

    ACE_TRY(d.set(dA, a.A, 2 * (size_t)mats * mn));
    L.A = dA;
    L.allow_i8 = i8;
    ACE_TRY(linops_setup(L, batch, st));
    if (i8 && !L.i8ok)
        return fail(ACE_ERR_UNSUPPORTED, "ace_linop_host: the codebook was not taken by the int8 digit-plane setup");
    if (L.pc_ok) return fail(ACE_ERR_UNSUPPORTED, "ace_linop_host: private code-image setup (not an operator path here)");

    if (op == ACE_LINOP_SETUP) {
        ACE_HIP(hipDeviceSynchronize());
        ACE_TRY(d.get(a.out, L.K, 2 * (size_t)mats * mm));
        ACE_TRY(d.get(a.out2, L.G, 2 * (size_t)mats * mm));
        if (a.out3) {
            double c[2] = {0.0, 0.0};
            if (i8) ACE_TRY(d.get(c, L.c8, 2));
            a.out3[0] = c[0];
            a.out3[1] = c[1];
        }
        return ACE_OK;
    }

    std::vector<RealState> rs((size_t)batch);
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    for (int b = 0; b < batch; ++b) {
        rs[b].mu = a.mu[b];
        rs[b].vbound = a.vbound ? a.vbound[b] : 0.0;
        rs[b].done = a.done ? a.done[b] : 0;
        rs[b].nzero = a.nzero ? a.nzero[b] : 0;
        rs[b].avok = a.avok ? a.avok[b] : 0;
    }
    ACE_TRY(d.set(drs, rs.data(), rs.size()));
    if (needZ) {
        ACE_TRY(d.set(dZ, a.Z, bn));
        ACE_TRY(d.set(dN, a.N, bn, 0.0));
    }
    if (needY) {
        ACE_TRY(d.set(dY, a.Y, bm));
        ACE_TRY(d.set(dM, a.M, bm, 0.0));
    }
    if (needg) ACE_TRY(d.set(dg, a.g, bm));
    if (a.AX) ACE_TRY(d.set(dAX, a.AX, bm));
    const size_t nout = (op == ACE_LINOP_AH) ? bn : bm;
    ACE_TRY(d.set(dout, nullptr, nout, a.sentinel));
    // the intermediates a launch_pre writes start from the sentinel too (a row it skips stays visible)
    ACE_TRY(d.set(dV, nullptr, bn, a.sentinel));
    ACE_TRY(d.set(dS, nullptr, bm, a.sentinel));

    switch (op) {
    case ACE_LINOP_A:   // T = (Y - M/mu) - A (Z - N/mu)
        if (i8 && r == 1) {
            launch_i8_apply_A(batch, n, m, L.LA8, dZ, dN, dY, dM, dout, L.c8, drs, dzeros, a.AX ? dAX : nullptr, st);
        } else if (path == ACE_LINOP_F64_FUSED) {
            launch_zgemm_fused(true, m, n, batch, L.A, n, dZ, dN, n, dout, dY, dM, m, drs, st);
        } else {
            launch_pre(n * r, m * r, batch, dZ, dN, dY, dM, i8 ? nullptr : dV, dS, drs, st);
            if (i8) launch_i8_apply_A(nv, n, m, L.LA8, dZ, dN, dY, dM, dout, L.c8, drs, dzeros, nullptr, st, r);
            else if (shared) launch_zgemm(1, false, m, n, nv, L.A, n, 0, dV, n, 0, dout, dS, m, 0, 1, st);
            else launch_zgemv_rows(1, m, n, batch, L.A, mn, dV, n, dout, dS, m, st);
        }
        break;
    case ACE_LINOP_AH:   // X = (Z - N/mu) + A^H g; the int8 rcols = 1 form returns W = A^H g
        if (i8 && r == 1) {
            launch_i8_apply_AH(batch, m, n, L.LAH8, dg, dout, L.c8, drs, st, nullptr);
        } else if (i8) {
            ZArgs zv{};
            zv.r = r;
            zv.xzn = 1;
            zv.Z = dZ;
            zv.N = dN;
            zv.zeros = dzeros;
            launch_i8_apply_AH(nv, m, n, L.LAH8, dg, dout, L.c8, drs, st, nullptr, &zv);
        } else if (path == ACE_LINOP_F64_FUSED) {
            launch_zgemm_fused(false, n, m, batch, L.AH, m, dg, nullptr, m, dout, dZ, dN, n, drs, st);
        } else {
            launch_pre(n * r, m * r, batch, dZ, dN, dY, dM, dV, dS, drs, st);
            if (shared) launch_zgemm(2, false, n, m, nv, L.AH, m, 0, dg, m, 0, dout, dV, n, 0, 1, st);
            else launch_zgemv_cols(2, m, n, batch, L.A, mn, dg, m, dout, dV, n, st);
        }
        break;
    case ACE_LINOP_K:
    case ACE_LINOP_G: {
        const double* Lm = op == ACE_LINOP_K ? L.K : L.G;
        if (i8) launch_i8_apply_K(nv, m, L.LK8, dg, dout, L.c8, drs, st, r);
        else if (shared) launch_zgemm(0, false, m, m, nv, Lm, m, 0, dg, m, 0, dout, nullptr, m, 0, 1, st);
        else launch_zgemv_rows(0, m, m, batch, Lm, mm, dg, m, dout, nullptr, m, st);
        break;
    }
    default: break;
    }
    ACE_LAUNCHED("ace_linop_host");
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(a.out, dout, nout));
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" {

int ace_linop_host(const ace_linop_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_linop_host: NULL arguments");
    return linop_run(*args);
}

int ace_zgemm_host(int mode, int conj_l, int M, int K, int nb, const double* L, long long nL, int ldl, long long strideL,
                   const double* V, long long nV, int ldv, long long strideV, double* C, const double* E, long long nC,
                   int ldc, long long strideC, int nz, const double* klim, long long nklim, long long klim_stride) {
    g_err.clear();
    if (mode < 0 || mode > 2 || M < 1 || K < 1 || nb < 1 || nz < 1 || !L || !V || !C || (mode != 0 && !E) || ldl < K ||
        ldv < K || ldc < M || strideL < 0 || strideV < 0 || strideC < 0 || klim_stride < 0)
        return fail(ACE_ERR_ARG, "ace_zgemm_host: bad arguments");
    // every element a launch may touch lies inside the caller's arrays (complex element counts)
    const long long z1 = nz - 1;
    if (z1 * strideL + (long long)(M - 1) * ldl + K > nL || z1 * strideV + (long long)(nb - 1) * ldv + K > nV ||
        z1 * strideC + (long long)(nb - 1) * ldc + M > nC || (klim && z1 * klim_stride + 1 > nklim))
        return fail(ACE_ERR_ARG, "ace_zgemm_host: operand extents exceed the given array sizes");
    DevScope d;
    double *dL, *dV, *dC, *dE = nullptr, *dk = nullptr;
    ACE_TRY(d.put(&dL, L, 2 * (size_t)nL));
    ACE_TRY(d.put(&dV, V, 2 * (size_t)nV));
    ACE_TRY(d.put(&dC, C, 2 * (size_t)nC));
    if (mode != 0) ACE_TRY(d.put(&dE, E, 2 * (size_t)nC));
    if (klim) ACE_TRY(d.put(&dk, klim, (size_t)nklim));
    launch_zgemm(mode, conj_l != 0, M, K, nb, dL, ldl, strideL, dV, ldv, strideV, dC, dE, ldc, strideC, nz, nullptr, dk,
                 klim_stride);
    ACE_LAUNCHED("ace_zgemm_host");
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(C, dC, 2 * (size_t)nC));
    return ACE_OK;
}

}  // extern "C"
