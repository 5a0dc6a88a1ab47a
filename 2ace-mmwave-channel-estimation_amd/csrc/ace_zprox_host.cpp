// Test entry for the Z-step of the ADMM iteration (ace_zprox_host): host arrays in, one launch_zstep
// (after launch_zlean where asked), host arrays out.
//
// Nothing is re-implemented here.  The ZArgs block is filled field by field the way admm_run fills it
// (ace_admm.cpp: the block before the init Z-step, then the per-iteration fields ahead of launch_zstep),
// one RealState per realisation is filled from the caller's state / flags (every other field zero), and
// the launcher picks the kernel as it does in a solve: zstep1w_kernel at r = 1, zstep_kernel otherwise.
// The Y-step sums and dual terms are the caller's (yfused = 1, as gyk_kernel leaves them); the four-wave
// kernel forms its dual terms from Y / K Y buffers, which are zero here.  The producers of the Z-step's
// inputs that carry solver state -- the fused apply_AH (xfuse) and the A2only m-space steady state (msp) -- have an
// entry of their own, ace_unit_host (ace_unit_host.cpp), which runs them with their fused control; the compact
// launch is not reachable.  The A2nuclear m-space state and its lazy dual residual (nms_kernel) have theirs:
// ace_nms_host (ace_nms_host.cpp).
#include "ace_host.hpp"

namespace ace {
namespace {

int zprox_run(const ace_zprox_args& a) {
    const int batch = a.batch, tx = a.tx, rx = a.rx, r = a.r, m = a.m;
    const bool init = a.init != 0, pp = a.pingpong != 0, wmode = a.wmode != 0;
    if (a.variant != ACE_VARIANT_A2ONLY && a.variant != ACE_VARIANT_NUCLEAR)
        return fail(ACE_ERR_ARG, "ace_zprox_host: unknown variant %d", a.variant);
    if (batch < 1 || batch > (1 << 20) || tx < 1 || tx > 32 || rx < 1 || rx > 32 || r < 1 || r > 32 || m < 1 || m > 4096)
        return fail(ACE_ERR_ARG, "ace_zprox_host: bad shape (batch %d, tx %d, rx %d, r %d, m %d)", batch, tx, rx, r, m);
    if (a.np < 0 || a.np > 4) return fail(ACE_ERR_ARG, "ace_zprox_host: rank profile length %d", a.np);
    for (int p = 0; p < a.np; ++p)
        if (a.rl[p] < 1 || a.rl[p] > tx || !(a.fl[p] > 0.0 && a.fl[p] < 1.0))
            return fail(ACE_ERR_ARG, "ace_zprox_host: rank profile entry %d (rank %d, share %g)", p, a.rl[p], a.fl[p]);
    if (!a.X) return fail(ACE_ERR_ARG, "ace_zprox_host: NULL X");
    if (!init && a.it < 1) return fail(ACE_ERR_ARG, "ace_zprox_host: iteration %d (the iterations count from 1)", a.it);
    if (!init && a.warm && !a.Q) return fail(ACE_ERR_ARG, "ace_zprox_host: a warm step needs Q");
    if (!(a.rho > 0.0)) return fail(ACE_ERR_ARG, "ace_zprox_host: rho %g", a.rho);
    if (tx < 2 || (tx & 1))
        return fail(ACE_ERR_UNSUPPORTED, "ace_zprox_host: the Z-step kernels take an even tx (the API pads odd tx)");
    if (wmode && (init || r != 1 || !pp))
        return fail(ACE_ERR_UNSUPPORTED, "ace_zprox_host: wmode is the r = 1 iteration form with ping-pong outputs");
    if (pp && !wmode) return fail(ACE_ERR_UNSUPPORTED, "ace_zprox_host: ping-pong outputs belong to wmode");
    if (wmode && !zstep_takes_w(a.variant, r))
        return fail(ACE_ERR_UNSUPPORTED, "ace_zprox_host: the selected Z-step kernel does not take W");
    if (a.lean && !(wmode && a.variant == ACE_VARIANT_A2ONLY && a.warm))
        return fail(ACE_ERR_UNSUPPORTED, "ace_zprox_host: the lean kernel runs before a warm A2only wmode step");

    const int n = tx * rx, nc = (r == 1 || a.row_mode) ? r : 1;
    const size_t bn = 2 * (size_t)batch * r * n, bm = 2 * (size_t)batch * r * m, bq = 2 * (size_t)batch * tx * tx;
    const size_t bo = 2 * (size_t)batch * nc * n;
    double *dX, *dZ, *dN, *dZ2, *dN2, *dQ, *doptX, *doptY, *dXcur, *dY, *dzeros;
    RealState* drs;
    int* ddone;
    unsigned char* dr1;
    auto carve = [&](Carver& cv) {
        dX = cv.take(8 * bn);
        dZ = cv.take(8 * bn);
        dN = cv.take(8 * bn);
        dZ2 = cv.take(8 * bn);
        dN2 = cv.take(8 * bn);
        dQ = cv.take(8 * bq);
        doptX = cv.take(8 * bo);
        dXcur = cv.take(8 * bn);
        doptY = cv.take(8 * bm);
        dY = cv.take(8 * bm);   // Y, Y_old, K Y, K Y_old of the four-wave kernel: one zero buffer
        dzeros = cv.take(16 * (size_t)n);
        drs = cv.take<RealState>(sizeof(RealState) * (size_t)batch);
        ddone = cv.take<int>(256);
        dr1 = cv.take<unsigned char>((size_t)batch);
    };
    DevScope d;
    ACE_TRY(carve_zeroed(d, carve));
    hipStream_t st = nullptr;

    std::vector<RealState> rs((size_t)batch);
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    for (int b = 0; b < batch; ++b) {
        RealState& s = rs[b];
        s.mu = 1.0;
        if (a.state) {
            const double* v = a.state + (size_t)b * ACE_ZP_NIN;
            s.mu = v[0];
            s.last_res = v[1];
            s.opt_obj = v[2];
            s.obj2 = v[3];
            s.nAX2 = v[4];
            s.nY2 = v[5];
            s.nJM2 = v[6];
            s.dY2 = v[7];
            s.dAtY = v[8];
            s.nAtY = v[9];
            s.kfcum = v[10];
            for (int p = 0; p < 4; ++p) s.kf[p] = v[11 + p];
        }
        if (a.flags) {
            const int32_t* f = a.flags + (size_t)b * ACE_ZP_NFLAG;
            s.done = f[0];
            s.nzero = f[1];
            s.kfok = f[2];
            s.optsrc = f[3];
        }
    }
    ACE_TRY(d.set(drs, rs.data(), rs.size()));
    ACE_TRY(d.set(dX, a.X, bn));
    ACE_TRY(d.set(dZ, a.Z, bn, 0.0));
    ACE_TRY(d.set(dN, a.N, bn, 0.0));
    ACE_TRY(d.set(dZ2, nullptr, bn, a.sentinel));
    ACE_TRY(d.set(dN2, nullptr, bn, a.sentinel));
    ACE_TRY(d.set(dQ, a.Q, bq, a.sentinel));
    ACE_TRY(d.set(doptX, nullptr, bo, a.sentinel));
    ACE_TRY(d.set(dXcur, nullptr, bn, a.sentinel));
    if (a.rank_one) ACE_TRY(d.set(dr1, a.rank_one, (size_t)batch));

    ZArgs za{};
    za.n = n;
    za.m = m;
    za.tx = tx;
    za.rx = rx;
    za.r = r;
    za.row_mode = (r == 1) ? 1 : (a.row_mode != 0);
    za.X = dX;
    za.N = dN;
    za.Z = dZ;
    za.Q = dQ;
    za.st = drs;
    za.optX = doptX;
    za.optY = doptY;
    za.done_count = ddone;
    if (a.np > 0) {
        za.np = a.np;
        for (int p = 0; p < a.np; ++p) {
            za.rl[p] = a.rl[p];
            za.fl[p] = a.fl[p];
        }
    } else {
        za.np = rank_profile(tx, rx, m, n, 0, za.rl, za.fl);
    }
    za.rank_one = a.rank_one ? dr1 : nullptr;
    za.tol_rel = a.tol_rel;
    za.tol_abs = a.tol_abs;
    za.rho = a.rho;
    za.fixed_iters = a.fixed_iters;
    za.warm = a.warm;
    za.zcert = a.zcert ? 1 : 0;
    za.r1lz = a.r1lz ? 1 : 0;
    za.tkeig = a.tkeig > 0 ? a.tkeig : 0;
    za.tkcnt = ddone + 32;
    za.Xcur = dXcur;
    za.zeros = dzeros;
    za.nuclear = a.variant == ACE_VARIANT_NUCLEAR;
    za.Kf = nullptr;
    if (init) {
        za.it = 0;
        launch_zstep(a.variant, true, za, batch, st);
    } else {
        za.it = a.it;
        za.wmode = wmode;
        if (pp) {
            za.Zn = dZ2;
            za.Nn = dN2;
        }
        za.yfused = 1;
        za.ytiles = (m + 63) / 64;
        za.Ynew = za.Yold = za.KYnew = za.KYold = dY;
        za.lean = a.lean ? 1 : 0;
        if (za.lean) launch_zlean(za, batch, st);
        launch_zstep(a.variant, false, za, batch, st);
    }
    ACE_LAUNCHED("ace_zprox_host");
    ACE_HIP(hipDeviceSynchronize());

    ACE_TRY(d.get(a.Zo, pp ? dZ2 : dZ, bn));
    ACE_TRY(d.get(a.No, pp ? dN2 : dN, bn));
    ACE_TRY(d.get(a.Qo, dQ, bq));
    ACE_TRY(d.get(a.optX, doptX, bo));
    ACE_TRY(d.get(a.Xcur, dXcur, bo));
    ACE_TRY(d.get(rs.data(), drs, rs.size()));
    for (int b = 0; b < batch; ++b) {
        const RealState& s = rs[b];
        if (a.state_out) {
            double* v = a.state_out + (size_t)b * ACE_ZP_NOUT;
            v[0] = s.mu;
            v[1] = s.last_res;
            v[2] = s.opt_obj;
            v[3] = s.vbound;
            for (int p = 0; p < 4; ++p) v[4 + p] = s.kf[p];
            v[8] = s.kfcum;
        }
        if (a.flags_out) {
            int32_t* f = a.flags_out + (size_t)b * ACE_ZP_NFLAGOUT;
            f[0] = s.iters;
            f[1] = s.done;
            f[2] = s.status;
            f[3] = s.nzero;
            f[4] = s.avok;
            f[5] = s.kfok;
            f[6] = s.optsrc;
            f[7] = s.zit;
        }
    }
    if (a.tkcnt) ACE_TRY(d.get(a.tkcnt, ddone + 32, 2));
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_zprox_host(const ace_zprox_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_zprox_host: NULL arguments");
    return zprox_run(*args);
}
