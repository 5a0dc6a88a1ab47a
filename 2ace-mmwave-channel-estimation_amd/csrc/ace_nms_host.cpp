// Test entry for the A2nuclear m-space iteration (ace_nms_host): host arrays in, one operation of
// ace_nucmsp.hip, host arrays out.
//
// Nothing is re-implemented here.  NmsArgs, ZArgs (lazy_dual = 1, r = 1) and DualCtl are filled the way
// admm_nuclear_msp fills them (ace_admm.cpp), one RealState per realisation is filled from the caller's state /
// flags (every other field zero), and the operation is the solve's own launcher: launch_nms_init, launch_gyk_gfrag
// of the caller's dense G and K followed by one launch_nms (step: an iteration; fin: only the pending convergence
// tests), launch_nms_out.  Every per-realisation vector buffer is followed by `guard` doubles of `sentinel`, and
// a buffer the caller does not supply starts from `sentinel` too, so that what a kernel left untouched can be
// asserted; the control blocks are followed by one guard block whose bytes are compared after the launch.
#include "ace_host.hpp"

namespace ace {
namespace {

const char* const kOps[ACE_NMS_NOPS] = {"init", "step", "fin", "out"};

int nms_run(const ace_nms_args& a) {
    const int op = a.op, batch = a.batch, n = a.n, m = a.m;
    if (op < 0 || op >= ACE_NMS_NOPS) return fail(ACE_ERR_ARG, "ace_nms_host: unknown op %d", op);
    const char* on = kOps[op];
    if (batch < 1 || batch > (1 << 16)) return fail(ACE_ERR_ARG, "ace_nms_host (%s): batch %d", on, batch);
    if (m < 1) return fail(ACE_ERR_ARG, "ace_nms_host (%s): m %d", on, m);
    if (m > GYK_MAXM)
        return fail(ACE_ERR_UNSUPPORTED, "ace_nms_host (%s): m = %d beyond the m-space kernels' %d", on, m, GYK_MAXM);
    if (n < 1 || n > (1 << 16)) return fail(ACE_ERR_ARG, "ace_nms_host (%s): n %d", on, n);
    if (a.guard < 0 || a.guard > (1 << 24)) return fail(ACE_ERR_ARG, "ace_nms_host (%s): guard %d", on, a.guard);
    const bool step = op == ACE_NMS_STEP, fin = op == ACE_NMS_FIN, iter = step || fin;
    if (iter && !(a.rho > 0.0)) return fail(ACE_ERR_ARG, "ace_nms_host (%s): rho %g", on, a.rho);
    if (step && a.it < 1)
        return fail(ACE_ERR_ARG, "ace_nms_host (%s): it %d (the iterations count from 1)", on, a.it);
#define NMS_NEED(cond, p) \
    if ((cond) && !a.p) return fail(ACE_ERR_ARG, "ace_nms_host (%s): NULL " #p, on)
    NMS_NEED(op == ACE_NMS_INIT || op == ACE_NMS_OUT, Xinit);
    NMS_NEED(op == ACE_NMS_INIT, P0);
    NMS_NEED(step, G);
    NMS_NEED(iter, K);
    NMS_NEED(iter, Yo);
    NMS_NEED(fin, Yn);
    NMS_NEED(step, M);
    NMS_NEED(step, B);
    NMS_NEED(step, Eo);
    NMS_NEED(step, AEo);
    NMS_NEED(op != ACE_NMS_INIT, state);
    NMS_NEED(iter, flags);
    NMS_NEED(op == ACE_NMS_OUT, optW);
    NMS_NEED(op == ACE_NMS_OUT, curW);
#undef NMS_NEED
    // (last: the budget query behind it is the first call that may touch the HIP runtime)
    if (!nms_supported(m))
        return fail(ACE_ERR_UNSUPPORTED, "ace_nms_host (%s): the kernels' LDS request at m = %d is refused", on, m);

    const size_t g = (size_t)a.guard, bm = 2 * (size_t)batch * m, bn = 2 * (size_t)batch * n;
    const size_t mm = 2 * (size_t)m * m;
    double *dG, *dK, *dGf, *dKf, *dX, *dP0, *dB, *dYo, *dYn, *dM, *dEo, *dEn, *dAEo, *dAEn, *doptW, *doptY, *dcurW;
    double *dV, *dWsel;
    RealState* drs;
    int* ddone;
    auto carve = [&](Carver& cv) {
        dG = cv.take(8 * mm);
        dK = cv.take(8 * mm);
        dGf = cv.take(gyk_gfrag_bytes(m));
        dKf = cv.take(gyk_gfrag_bytes(m));
        dX = cv.take(8 * bn);
        dP0 = cv.take(8 * bm);
        dB = cv.take(8 * ((size_t)batch * m + g));
        double** vb[] = {&dYo, &dYn, &dM, &dEo, &dEn, &dAEo, &dAEn, &doptW, &doptY, &dcurW, &dWsel};
        for (double** p : vb) *p = cv.take(8 * (bm + g));
        dV = cv.take(8 * (bn + g));
        drs = cv.take<RealState>(sizeof(RealState) * ((size_t)batch + 1));
        ddone = cv.take<int>(256);
    };
    DevScope d;
    ACE_TRY(carve_zeroed(d, carve));
    hipStream_t st = nullptr;

    std::vector<RealState> rs((size_t)batch + 1);
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    memset(&rs[batch], 0x5A, sizeof(RealState));   // the guard block
    for (int b = 0; b < batch; ++b) {
        RealState& s = rs[b];
        s.mu = 1.0;
        if (a.state) {
            const double* v = a.state + (size_t)b * ACE_NMS_NSTATE;
            s.mu = v[0];
            s.last_res = v[1];
            s.opt_obj = v[2];
            s.na = v[3];
            s.naz = v[4];
            s.nbeta = v[5];
            s.nep2 = v[6];
            s.nopt_a = v[7];
            s.ncur_a = v[8];
            s.pd_dZ2 = v[9];
            s.pd_nZ2 = v[10];
            s.pd_rc = v[11];
            s.obj2 = v[12];
            s.nAX2 = v[13];
            s.nY2 = v[14];
            s.nJM2 = v[15];
            s.dY2 = v[16];
            s.dAtY = v[17];
            s.nAtY = v[18];
            s.nx0 = v[19];
        }
        if (a.flags) {
            const int32_t* f = a.flags + (size_t)b * ACE_NMS_NFLAG;
            s.iters = f[0];
            s.done = f[1];
            s.status = f[2];
            s.dpend = f[3];
        }
    }
    const std::vector<RealState> rs_in = rs;
    ACE_TRY(d.set(drs, rs.data(), rs.size()));
    ACE_TRY(d.set(ddone, &a.done_count, 1));
    // a vector buffer: the caller's rows (or `sentinel`), then the guard
    auto load = [&](double* dst, const double* src, size_t count) -> int {
        ACE_TRY(d.set(dst, src, count, a.sentinel));
        return d.set(dst + count, nullptr, g, a.sentinel);
    };
    if (a.G) ACE_TRY(d.set(dG, a.G, mm));
    if (a.K) ACE_TRY(d.set(dK, a.K, mm));
    if (a.Xinit) ACE_TRY(d.set(dX, a.Xinit, bn));
    if (a.P0) ACE_TRY(d.set(dP0, a.P0, bm));
    ACE_TRY(load(dB, a.B, (size_t)batch * m));
    ACE_TRY(load(dYo, a.Yo, bm));
    ACE_TRY(load(dYn, a.Yn, bm));
    ACE_TRY(load(dM, a.M, bm));
    ACE_TRY(load(dEo, a.Eo, bm));
    ACE_TRY(load(dEn, nullptr, bm));
    ACE_TRY(load(dAEo, a.AEo, bm));
    ACE_TRY(load(dAEn, nullptr, bm));
    ACE_TRY(load(doptW, a.optW, bm));
    ACE_TRY(load(doptY, a.optY, bm));
    ACE_TRY(load(dcurW, a.curW, bm));
    ACE_TRY(load(dWsel, nullptr, bm));
    ACE_TRY(load(dV, nullptr, bn));

    NmsArgs na{};
    na.Gf = dGf;
    na.Kf = dKf;
    na.B = dB;
    na.Yo = dYo;
    na.Yn = dYn;
    na.M = dM;
    na.Eo = dEo;
    na.En = dEn;
    na.AEo = dAEo;
    na.AEn = dAEn;
    na.P0 = dP0;
    na.optW = doptW;
    na.optY = doptY;
    na.curW = dcurW;
    na.rs = drs;
    na.dc = DualCtl{a.tol_abs, a.tol_rel, a.rho, a.fixed_iters, n, 1, ddone};
    ZArgs za{};
    za.n = n;
    za.m = m;
    za.r = 1;
    za.row_mode = 1;
    za.st = drs;
    za.done_count = ddone;
    za.tol_rel = a.tol_rel;
    za.tol_abs = a.tol_abs;
    za.rho = a.rho;
    za.fixed_iters = a.fixed_iters;
    za.nuclear = 1;
    za.lazy_dual = 1;
    za.it = a.it;
    switch (op) {
        case ACE_NMS_INIT: launch_nms_init(batch, n, m, dX, na, st); break;
        case ACE_NMS_STEP:
            launch_gyk_gfrag(m, dG, dGf, st);
            launch_gyk_gfrag(m, dK, dKf, st);
            launch_nms(batch, m, na, za, false, st);
            break;
        case ACE_NMS_FIN:
            launch_gyk_gfrag(m, dK, dKf, st);
            launch_nms(batch, m, na, za, true, st);
            break;
        default: launch_nms_out(batch, n, m, dX, na, dV, dWsel, st); break;
    }
    ACE_LAUNCHED("ace_nms_host");
    ACE_HIP(hipDeviceSynchronize());

    ACE_TRY(d.get(a.B_out, dB, (size_t)batch * m + g));
    ACE_TRY(d.get(a.Yo_out, dYo, bm + g));
    ACE_TRY(d.get(a.Yn_out, dYn, bm + g));
    ACE_TRY(d.get(a.M_out, dM, bm + g));
    ACE_TRY(d.get(a.Eo_out, dEo, bm + g));
    ACE_TRY(d.get(a.En_out, dEn, bm + g));
    ACE_TRY(d.get(a.AEo_out, dAEo, bm + g));
    ACE_TRY(d.get(a.AEn_out, dAEn, bm + g));
    ACE_TRY(d.get(a.optW_out, doptW, bm + g));
    ACE_TRY(d.get(a.optY_out, doptY, bm + g));
    ACE_TRY(d.get(a.curW_out, dcurW, bm + g));
    ACE_TRY(d.get(a.Wsel, dWsel, bm + g));
    ACE_TRY(d.get(a.V, dV, bn + g));
    ACE_TRY(d.get(rs.data(), drs, rs.size()));
    for (int b = 0; b < batch; ++b) {
        const RealState& s = rs[b];
        if (a.state_out) {
            double* v = a.state_out + (size_t)b * ACE_NMS_NSTATE;
            v[0] = s.mu;
            v[1] = s.last_res;
            v[2] = s.opt_obj;
            v[3] = s.na;
            v[4] = s.naz;
            v[5] = s.nbeta;
            v[6] = s.nep2;
            v[7] = s.nopt_a;
            v[8] = s.ncur_a;
            v[9] = s.pd_dZ2;
            v[10] = s.pd_nZ2;
            v[11] = s.pd_rc;
            v[12] = s.obj2;
            v[13] = s.nAX2;
            v[14] = s.nY2;
            v[15] = s.nJM2;
            v[16] = s.dY2;
            v[17] = s.dAtY;
            v[18] = s.nAtY;
            v[19] = s.nx0;
        }
        if (a.flags_out) {
            int32_t* f = a.flags_out + (size_t)b * ACE_NMS_NFLAG;
            f[0] = s.iters;
            f[1] = s.done;
            f[2] = s.status;
            f[3] = s.dpend;
        }
    }
    if (a.done_count_out) ACE_TRY(d.get(a.done_count_out, ddone, 1));
    if (a.guard_ok) {
        // the guard block, and every control-block field the entry does not carry (all zero on entry)
        const RealState z{};
        int ok = memcmp(&rs[batch], &rs_in[batch], sizeof(RealState)) == 0;
        for (int b = 0; b < batch && ok; ++b) {
            const RealState& s = rs[b];
            ok = s.nB == 0.0 && s.vbound == 0.0 && s.objcol == 0 && s.nzero == 0 && s.optsrc == 0 && s.avok == 0 &&
                 s.optysrc == 0 && memcmp(s.kf, z.kf, sizeof s.kf) == 0 && s.kfcum == 0.0 && s.kfok == 0 && s.zit == 0 &&
                 s.fzit == 0 && s.fs0 == 0.0 && s.fs3 == 0.0 && s.msp == 0 && s.mzit == 0 && s.z0id == 0 &&
                 s.msp_pad == 0 && s.mres == 0 && s.npad2_ == 0.0;
        }
        *a.guard_ok = ok;
    }
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_nms_host(const ace_nms_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_nms_host: NULL arguments");
    return nms_run(*args);
}
