// Test entry for the private code-image kernels (ace_pc_host): host arrays in, one operation of
// ace_private.hip, host arrays out.
//
// Nothing is re-implemented here.  Every operation calls the launchers a solve calls (launch_pc_pack, the three
// steps of launch_pc_ginv, launch_pc_apply_a, launch_pgk), PgkArgs is filled the way admm_run fills it
// (ace_admm.cpp) and one RealState per realisation is filled from the caller's state / flags (every other field
// zero).  Every device buffer a kernel writes starts from `sentinel` and is followed by `guard` doubles (dwords
// for the code images) of it; the code images start from 0xFF bytes, as the solve hands these kernels a workspace
// nobody clears: a kernel that consumes a dword pc_pack never wrote shows up in a product.  The control blocks are
// followed by one guard block whose bytes are compared after the launch.
#include "ace_host.hpp"

namespace ace {
namespace {

const char* const kOps[ACE_PC_NOPS] = {"pack", "kmat", "inv", "tiles", "apply_a", "step"};

// the dimensions of ace_private.hip::pc_dims that size the buffers here
struct Dims {
    size_t mt, mp32, ntile, nH, nA, nR;   // nH, nA, nR: dwords of one realisation's three images
};
Dims dims_of(int m, int n) {
    Dims d;
    d.mt = ((size_t)m + 15) / 16;
    d.mp32 = 32 * (((size_t)m + 31) / 32);
    d.ntile = d.mt * (d.mt + 1) / 2;
    const size_t nct = ((size_t)n + 15) / 16;
    d.nH = nct * ((d.mt + 7) / 8) * 128;
    d.nA = d.mt * ((nct + 7) / 8) * 128;
    d.nR = (size_t)m * nct;
    return d;
}

int pc_run(const ace_pc_args& a) {
    const int op = a.op, batch = a.batch, m = a.m, n = a.n;
    if (op < 0 || op >= ACE_PC_NOPS) return fail(ACE_ERR_ARG, "ace_pc_host: unknown op %d", op);
    const char* on = kOps[op];
    if (batch < 1 || batch > (1 << 12)) return fail(ACE_ERR_ARG, "ace_pc_host (%s): batch %d", on, batch);
    if (m < 1) return fail(ACE_ERR_ARG, "ace_pc_host (%s): m %d", on, m);
    if (n < 1) return fail(ACE_ERR_ARG, "ace_pc_host (%s): n %d", on, n);
    if (m > PC_MAXM)
        return fail(ACE_ERR_UNSUPPORTED, "ace_pc_host (%s): m = %d beyond the code-image kernels' %d", on, m, PC_MAXM);
    if (n > PC_MAXN)
        return fail(ACE_ERR_UNSUPPORTED, "ace_pc_host (%s): n = %d beyond the code-image kernels' %d", on, n, PC_MAXN);
    if (a.guard < 0 || a.guard > (1 << 24)) return fail(ACE_ERR_ARG, "ace_pc_host (%s): guard %d", on, a.guard);
    const bool pack = op == ACE_PC_PACK, kmat = op == ACE_PC_KMAT, inv = op == ACE_PC_INV, tiles = op == ACE_PC_TILES;
    const bool apply = op == ACE_PC_APPLY_A, step = op == ACE_PC_STEP;
    if (inv && (a.form < 0 || a.form >= ACE_PC_NFORMS))
        return fail(ACE_ERR_ARG, "ace_pc_host (%s): unknown form %d", on, a.form);
    if (step && (a.yn_id < 0 || a.yn_id > 2)) return fail(ACE_ERR_ARG, "ace_pc_host (%s): yn_id %d", on, a.yn_id);
#define PC_NEED(cond, p) \
    if ((cond) && !a.p) return fail(ACE_ERR_ARG, "ace_pc_host (%s): NULL " #p, on)
    PC_NEED(pack || kmat || apply || step, A);
    PC_NEED(inv || tiles, Gin);
    PC_NEED(apply, X0);
    PC_NEED(step, B);
    PC_NEED(step, Yo);
    PC_NEED(step, M);
    PC_NEED(step, Z);
    PC_NEED(step, N);
    PC_NEED(step, state);
    PC_NEED(step, flags);
#undef PC_NEED
    if (step)
        for (int b = 0; b < batch; ++b)
            if (!(a.state[(size_t)b * ACE_PC_NSTATE] > 0.0))
                return fail(ACE_ERR_ARG, "ace_pc_host (%s): mu %g of realisation %d", on,
                            a.state[(size_t)b * ACE_PC_NSTATE], b);
    if (!pc_supported(m, n))
        return fail(ACE_ERR_UNSUPPORTED, "ace_pc_host (%s): pgk_kernel's LDS request at m = %d, n = %d is refused", on, m,
                    n);

    const Dims dm = dims_of(m, n);
    const size_t g = (size_t)a.guard, bm = 2 * (size_t)batch * m, bn = 2 * (size_t)batch * n;
    const size_t ncode = (size_t)batch * (dm.nH + dm.nA + dm.nR);            // dwords
    const size_t ngw = (size_t)batch * pc_gw_bytes(m) / 8;                   // doubles: matrices, then the scratch
    const size_t nmat = 2 * (size_t)batch * dm.mp32 * dm.mp32, ngt = (size_t)batch * dm.ntile * 512;
    if (ncode * 4 != (size_t)batch * pc_codes_bytes(m, n) || ngt * 8 != (size_t)batch * pc_gt_bytes(m))
        return fail(ACE_ERR_WORKSPACE, "ace_pc_host: the entry's buffer sizes differ from the kernels'");
    double *dA, *dcb, *dGw, *dGt, *dX0, *dP0, *dB, *dYo, *dM, *dAX, *dYn, *doptY, *dW, *dZ, *dN, *dzeros;
    uint32_t* dcodes;
    int* dflag;
    RealState* drs;
    auto carve = [&](Carver& cv) {
        dA = cv.take(16 * (size_t)batch * m * n);
        dcb = cv.take(8 * ((size_t)batch + g));
        dcodes = cv.take<uint32_t>(4 * (ncode + g));
        dflag = cv.take<int>(256);
        dGw = cv.take(8 * (ngw + g));
        dGt = cv.take(8 * (ngt + g));
        dX0 = cv.take(8 * bn);
        dB = cv.take(8 * ((size_t)batch * m + g));
        double** vb[] = {&dP0, &dYo, &dM, &dAX, &dYn, &doptY};
        for (double** p : vb) *p = cv.take(8 * (bm + g));
        double** nb[] = {&dW, &dZ, &dN};
        for (double** p : nb) *p = cv.take(8 * (bn + g));
        dzeros = cv.take(16 * (size_t)n);
        drs = cv.take<RealState>(sizeof(RealState) * ((size_t)batch + 1));
    };
    DevScope d;
    ACE_TRY(carve_zeroed(d, carve));
    hipStream_t st = nullptr;

    auto load = [&](double* dst, const double* src, size_t count) -> int {
        ACE_TRY(d.set(dst, src, count, a.sentinel));
        return d.set(dst + count, nullptr, g, a.sentinel);
    };
    if (a.A) ACE_TRY(d.set(dA, a.A, 2 * (size_t)batch * m * n));
    ACE_TRY(load(dcb, nullptr, (size_t)batch));
    ACE_HIP(hipMemset(dcodes, 0xFF, 4 * (ncode + g)));
    ACE_TRY(load(dGw, nullptr, ngw));
    ACE_TRY(load(dGt, nullptr, ngt));
    if (a.Gin) ACE_TRY(d.set(dGw, a.Gin, nmat));
    if (a.X0) ACE_TRY(d.set(dX0, a.X0, bn));
    ACE_TRY(load(dP0, nullptr, bm));
    ACE_TRY(load(dB, a.B, (size_t)batch * m));
    ACE_TRY(load(dYo, a.Yo, bm));
    ACE_TRY(load(dM, a.M, bm));
    ACE_TRY(load(dAX, a.AX, bm));
    ACE_TRY(load(dYn, a.Yn, bm));
    ACE_TRY(load(doptY, a.optY, bm));
    ACE_TRY(load(dW, nullptr, bn));
    ACE_TRY(load(dZ, a.Z, bn));
    ACE_TRY(load(dN, a.N, bn));

    std::vector<RealState> rs((size_t)batch + 1);
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    memset(&rs[batch], 0x5A, sizeof(RealState));   // the guard block
    for (int b = 0; b < batch; ++b) {
        RealState& s = rs[b];
        s.mu = 1.0;
        if (a.state) {
            const double* v = a.state + (size_t)b * ACE_PC_NSTATE;
            s.mu = v[0];
            s.opt_obj = v[1];
            s.vbound = v[2];
            s.obj2 = v[3];
            s.nAX2 = v[4];
            s.nY2 = v[5];
            s.nJM2 = v[6];
            s.dY2 = v[7];
            s.dAtY = v[8];
            s.nAtY = v[9];
        }
        if (a.flags) {
            const int32_t* f = a.flags + (size_t)b * ACE_PC_NFLAG;
            s.done = f[0];
            s.avok = f[1];
            s.nzero = f[2];
            s.optysrc = f[3];
        }
    }
    const std::vector<RealState> rs_in = rs;
    ACE_TRY(d.set(drs, rs.data(), rs.size()));

    uint32_t* dcA = dcodes + pc_codesA_off(batch, m, n);
    if (!inv && !tiles) launch_pc_pack(batch, m, n, dA, dcb, dcodes, dflag, st);
    switch (op) {
        case ACE_PC_PACK: break;
        case ACE_PC_KMAT: launch_pc_k(batch, m, n, dcodes + (size_t)batch * (dm.nH + dm.nA), dcb, dGw, st); break;
        case ACE_PC_INV: launch_pc_inv(batch, m, dGw, a.form == ACE_PC_GJ ? PC_INV_GJ : PC_INV_SCHUR, st); break;
        case ACE_PC_TILES: launch_pc_tiles(batch, m, dGw, dGt, st); break;
        case ACE_PC_APPLY_A: launch_pc_apply_a(batch, m, n, dcA, dcb, dX0, dP0, st); break;
        default: {
            if (a.G) {   // the caller's dense G_b [m][m] in the setup's mp32 x mp32 frame, then its lower tiles
                std::vector<double> gw(nmat, a.sentinel);
                for (int b = 0; b < batch; ++b)
                    for (int i = 0; i < m; ++i)
                        memcpy(&gw[2 * (((size_t)b * dm.mp32 + i) * dm.mp32)], a.G + 2 * ((size_t)b * m + i) * m,
                               16 * (size_t)m);
                ACE_TRY(d.set(dGw, gw.data(), nmat));
                launch_pc_tiles(batch, m, dGw, dGt, st);
            } else {
                launch_pc_ginv(batch, m, n, dcodes, dcb, dGw, dGt, st);
            }
            const PgkArgs pa{m, n, dcodes, dcA, dGt, dcb, dB, dYo, dM,
                             dYn, dW, doptY, drs, dAX, a.yn_id, dZ, dN, dzeros};
            launch_pgk(batch, pa, st);
        }
    }
    ACE_LAUNCHED("ace_pc_host");
    ACE_HIP(hipDeviceSynchronize());

    ACE_TRY(d.get(a.cb, dcb, (size_t)batch + g));
    ACE_TRY(d.get(a.flag_out, dflag, 1));
    ACE_TRY(d.get(a.codes, dcodes, ncode + g));
    ACE_TRY(d.get(a.Gw, dGw, nmat));
    if (a.Gw) ACE_TRY(d.get(a.Gw + nmat, dGw + ngw, g));   // (the guard follows the recursion's scratch)
    ACE_TRY(d.get(a.Gt, dGt, ngt + g));
    ACE_TRY(d.get(a.P0, dP0, bm + g));
    ACE_TRY(d.get(a.B_out, dB, (size_t)batch * m + g));
    ACE_TRY(d.get(a.Yo_out, dYo, bm + g));
    ACE_TRY(d.get(a.M_out, dM, bm + g));
    ACE_TRY(d.get(a.AX_out, dAX, bm + g));
    ACE_TRY(d.get(a.Yn_out, dYn, bm + g));
    ACE_TRY(d.get(a.optY_out, doptY, bm + g));
    ACE_TRY(d.get(a.W, dW, bn + g));
    ACE_TRY(d.get(a.Z_out, dZ, bn + g));
    ACE_TRY(d.get(a.N_out, dN, bn + g));
    ACE_TRY(d.get(rs.data(), drs, rs.size()));
    for (int b = 0; b < batch; ++b) {
        const RealState& s = rs[b];
        if (a.state_out) {
            double* v = a.state_out + (size_t)b * ACE_PC_NSTATE;
            v[0] = s.mu;
            v[1] = s.opt_obj;
            v[2] = s.vbound;
            v[3] = s.obj2;
            v[4] = s.nAX2;
            v[5] = s.nY2;
            v[6] = s.nJM2;
            v[7] = s.dY2;
            v[8] = s.dAtY;
            v[9] = s.nAtY;
        }
        if (a.flags_out) {
            int32_t* f = a.flags_out + (size_t)b * ACE_PC_NFLAG;
            f[0] = s.done;
            f[1] = s.avok;
            f[2] = s.nzero;
            f[3] = s.optysrc;
        }
    }
    if (a.guard_ok) {
        // the guard block, and every control-block field the entry does not carry (all zero on entry)
        const RealState z{};
        int ok = memcmp(&rs[batch], &rs_in[batch], sizeof(RealState)) == 0;
        for (int b = 0; b < batch && ok; ++b) {
            const RealState& s = rs[b];
            ok = s.last_res == 0.0 && s.nB == 0.0 && s.iters == 0 && s.status == 0 && s.objcol == 0 && s.optsrc == 0 &&
                 memcmp(s.kf, z.kf, sizeof s.kf) == 0 && s.kfcum == 0.0 && s.kfok == 0 && s.zit == 0 &&
                 s.pd_dZ2 == 0.0 && s.pd_nZ2 == 0.0 && s.pd_rc == 0.0 && s.dpend == 0 && s.fzit == 0 && s.fs0 == 0.0 &&
                 s.fs3 == 0.0 && s.msp == 0 && s.mzit == 0 && s.z0id == 0 && s.msp_pad == 0 && s.mres == 0 &&
                 s.na == 0.0 && s.nbeta == 0.0 && s.nx0 == 0.0 && s.nopt_a == 0.0 && s.ncur_a == 0.0 && s.naz == 0.0 &&
                 s.nep2 == 0.0 && s.npad2_ == 0.0;
        }
        *a.guard_ok = ok;
    }
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_pc_host(const ace_pc_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_pc_host: NULL arguments");
    return pc_run(*args);
}
