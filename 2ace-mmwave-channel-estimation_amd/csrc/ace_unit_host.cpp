// Test entry for the unit path's fused iteration kernels (ace_unit_host): host arrays in, one launcher call of
// ace_i8gemm.hip, host arrays out.
//
// Nothing is re-implemented here.  The operators come from the caller's phase-code A through linops_carve /
// linops_setup (allow_i8) as in a solve: LA8, LAH8, LK8, c8 and Gf.  GykArgs, ZArgs, DualCtl and MsrArgs are filled
// field by field the way admm_iterate_split fills them at iteration `it` (ace_admm.cpp: the ping-pong choices by
// it & 1 and q, yn_id = 2 - q, Sold / Snew, fixup_now = (it == maxiter); the counters at the solve's offsets of its
// `done` block), one RealState per realisation is filled from the caller's state / flags (every other field zero),
// and the operation is one of the solve's launcher calls: launch_gyk, launch_gyf, launch_i8_apply_AH with the fused
// epilogue, launch_msr, launch_msr_ready, launch_i8_msp_optx.  Every per-realisation buffer is followed by `guard`
// doubles of `sentinel`, and a buffer the caller does not supply starts from `sentinel` too, so that what a kernel
// left untouched can be asserted; the control blocks are followed by one guard block whose bytes are compared after
// the launch.  The f64 K and G of the setup and c8 go back in the same call, so that a reference multiplies by the
// values the kernels multiply by.
#include "ace_host.hpp"

namespace ace {
namespace {

const char* const kOps[ACE_UNIT_NOPS] = {"gyk", "gyf", "ahf", "msr", "ready", "optx"};

int unit_run(const ace_unit_args& a) {
    const int op = a.op, batch = a.batch, n = a.n, m = a.m, it = a.it, q = a.q;
    if (op < 0 || op >= ACE_UNIT_NOPS) return fail(ACE_ERR_ARG, "ace_unit_host: unknown op %d", op);
    const char* on = kOps[op];
    if (batch < 1 || batch > (1 << 16)) return fail(ACE_ERR_ARG, "ace_unit_host (%s): batch %d", on, batch);
    if (m < 1) return fail(ACE_ERR_ARG, "ace_unit_host (%s): m %d", on, m);
    if (m > GYK_MAXM)
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (%s): m = %d beyond the fused kernels' %d", on, m, GYK_MAXM);
    if (n < 1 || n > 4096) return fail(ACE_ERR_ARG, "ace_unit_host (%s): n %d", on, n);
    if (a.guard < 0 || a.guard > (1 << 24)) return fail(ACE_ERR_ARG, "ace_unit_host (%s): guard %d", on, a.guard);
    const bool gyk = op == ACE_UNIT_GYK, gyf = op == ACE_UNIT_GYF, ahf = op == ACE_UNIT_AHF, msr = op == ACE_UNIT_MSR;
    const bool ready = op == ACE_UNIT_READY, optx = op == ACE_UNIT_OPTX, iter = gyk || gyf || ahf || msr;
    if ((iter || ready) && it < 1)
        return fail(ACE_ERR_ARG, "ace_unit_host (%s): it %d (the iterations count from 1)", on, it);
    if (iter && q != 0 && q != 1) return fail(ACE_ERR_ARG, "ace_unit_host (%s): q %d (0 or 1)", on, q);
    if (iter && !(a.rho > 0.0)) return fail(ACE_ERR_ARG, "ace_unit_host (%s): rho %g", on, a.rho);
    if (iter && (a.np < 0 || a.np > 4)) return fail(ACE_ERR_ARG, "ace_unit_host (%s): np %d (rank profile length)", on, a.np);
    if (msr && m != 256)
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (msr): m = %d (the m-space run takes m = 256)", m);
    if (msr && a.it_end <= it) return fail(ACE_ERR_ARG, "ace_unit_host (msr): it_end %d <= it %d", a.it_end, it);
    if (msr && a.waves != 8 && a.waves != 4) return fail(ACE_ERR_ARG, "ace_unit_host (msr): waves %d (8 or 4)", a.waves);
    const bool la = gyf || (gyk && a.use_la), ax = gyf || (gyk && a.use_ax), lazy = gyf || (gyk && a.lazy);
    const int zodd = it & 1;                       // Z, N of the previous iterate: Zb1 / Nb1 at odd iterations
    const int pm = (it - 1) & 1;                   // (msr) the buffers holding iterate it - 1
#define UNIT_NEED(cond, p) \
    if ((cond) && !a.p) return fail(ACE_ERR_ARG, "ace_unit_host (%s): NULL " #p, on)
    UNIT_NEED(!ready, A);
    UNIT_NEED(gyk || gyf || msr, B);
    UNIT_NEED(gyk && !la, T);
    UNIT_NEED(ahf, g);
    UNIT_NEED(((gyk || gyf) && q == 0) || (msr && pm == 0), Y0);
    UNIT_NEED(((gyk || gyf) && q == 1) || (msr && pm == 1), Y1);
    UNIT_NEED(gyk || gyf || msr, M);
    UNIT_NEED(msr, AX);
    UNIT_NEED(msr && pm == 0, S0);
    UNIT_NEED(msr && pm == 1, S1);
    UNIT_NEED(((la || ahf) && zodd) || optx, Zb1);
    UNIT_NEED(((la || ahf) && !zodd) || optx, Zb2);
    UNIT_NEED(true, flags);
#undef UNIT_NEED
    // (last: the budget queries are the first calls that may touch the HIP runtime)
    if (gyk && !lds_ok_budget(gyk_budget(), gyk_lds_bytes(m)))
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (gyk): gyk_kernel's LDS request at m = %d is refused", m);
    if (gyf && !lds_ok_budget(gyf_budget(), gyf_lds_bytes(m)))
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (gyf): gyf_kernel's LDS request at m = %d is refused", m);
    if (ahf && !lds_ok_budget(i8ah_budget(1), i8ah_lds_bytes(m) + i8ah_fuse_lds_bytes()))
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (ahf): the fused apply_AH's LDS request at m = %d is refused", m);
    if (optx && !lds_ok_budget(i8ah_budget(0), i8ah_lds_bytes(m)))
        return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (optx): apply_AH's LDS request at m = %d is refused", m);

    // state_ext: the rows of state / state_out carry RealState::recert as one more trailing element, and gyf_kernel
    // may raise the request (GykArgs::recert); 0: the rows and the launch as before the field existed
    const size_t nstate = ACE_UNIT_NSTATE + (a.state_ext ? 1 : 0);
    const size_t g = (size_t)a.guard, bm = 2 * (size_t)batch * m, bn = 2 * (size_t)batch * n;
    const size_t mm = 2 * (size_t)m * m, mn = 2 * (size_t)m * n;
    LinOps L{};
    double *dA, *dB, *dT, *dg, *dY[2], *dKY[2], *dM, *dAX, *doptY, *dS[2], *doptS, *dZ[2], *dN[2], *dX, *dXcur, *doptX;
    double* dzeros;
    unsigned char* dr1;
    RealState* drs;
    int* ddone;
    auto carve = [&](Carver& cv) {
        if (!ready) linops_carve(cv, true, batch, m, n, &L);
        dA = cv.take(8 * mn);
        dB = cv.take(8 * ((size_t)batch * m + g));
        double** vm[] = {&dT, &dg, &dY[0], &dY[1], &dKY[0], &dKY[1], &dM, &dAX, &doptY, &dS[0], &dS[1], &doptS};
        for (double** p : vm) *p = cv.take(8 * (bm + g));
        double** vn[] = {&dZ[0], &dZ[1], &dN[0], &dN[1], &dX, &dXcur, &doptX};
        for (double** p : vn) *p = cv.take(8 * (bn + g));
        dzeros = cv.take(16 * (size_t)n);
        dr1 = cv.take<unsigned char>((size_t)batch);
        drs = cv.take<RealState>(sizeof(RealState) * ((size_t)batch + 1));
        ddone = cv.take<int>(256);
    };
    DevScope d;
    ACE_TRY(carve_zeroed(d, carve));
    hipStream_t st = nullptr;

    if (!ready) {
        ACE_TRY(d.set(dA, a.A, mn));
        L.A = dA;
        L.allow_i8 = true;
        ACE_TRY(linops_setup(L, batch, st));
        if (!L.i8ok || !L.gyk_ok || !L.Gf)
            return fail(ACE_ERR_UNSUPPORTED, "ace_unit_host (%s): the codebook was not taken by the int8 digit-plane setup", on);
        ACE_HIP(hipDeviceSynchronize());
        ACE_TRY(d.get(a.K_out, L.K, mm));
        ACE_TRY(d.get(a.G_out, L.G, mm));
        ACE_TRY(d.get(a.c_out, L.c8, 2));
    }

    std::vector<RealState> rs((size_t)batch + 1);
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    memset(&rs[batch], 0x5A, sizeof(RealState));   // the guard block
    for (int b = 0; b < batch; ++b) {
        RealState& s = rs[b];
        s.mu = 1.0;
        if (a.state) {
            const double* v = a.state + (size_t)b * nstate;
            if (a.state_ext) s.recert = (int32_t)v[ACE_UNIT_NSTATE];
            s.mu = v[0];
            s.last_res = v[1];
            s.opt_obj = v[2];
            s.nB = v[3];
            s.vbound = v[4];
            s.obj2 = v[5];
            s.nAX2 = v[6];
            s.nY2 = v[7];
            s.nJM2 = v[8];
            s.dY2 = v[9];
            s.dAtY = v[10];
            s.nAtY = v[11];
            for (int p = 0; p < 4; ++p) s.kf[p] = v[12 + p];
            s.kfcum = v[16];
            s.pd_dZ2 = v[17];
            s.pd_nZ2 = v[18];
            s.pd_rc = v[19];
            s.fs0 = v[20];
            s.fs3 = v[21];
        }
        const int32_t* f = a.flags + (size_t)b * ACE_UNIT_NFLAG;
        s.iters = f[0];
        s.done = f[1];
        s.status = f[2];
        s.nzero = f[3];
        s.avok = f[4];
        s.optsrc = f[5];
        s.optysrc = f[6];
        s.kfok = f[7];
        s.dpend = f[8];
        s.fzit = f[9];
        s.zit = f[10];
        s.mzit = f[11];
        s.msp = f[12];
        s.z0id = f[13];
        s.msp_pad = f[14];
        s.mres = f[15];
    }
    const std::vector<RealState> rs_in = rs;
    ACE_TRY(d.set(drs, rs.data(), rs.size()));
    // the solve's counters at their offsets of AdmmState::done: [0] stopped realisations, [1] m-space steps, [8] the
    // run's resume point, [12..15] its step counts, [28..30] the readiness counts, [40] m-vectors written
    int cnt[64] = {};
    cnt[0] = a.done_count;
    cnt[1] = a.mspcount;
    cnt[8] = a.it_end;
    ACE_TRY(d.set(ddone, cnt, 64));
    if (a.rank_one) ACE_TRY(d.set(dr1, a.rank_one, (size_t)batch));
    // a vector buffer: the caller's rows (or `sentinel`), then the guard
    auto load = [&](double* dst, const double* src, size_t count) -> int {
        ACE_TRY(d.set(dst, src, count, a.sentinel));
        return d.set(dst + count, nullptr, g, a.sentinel);
    };
    ACE_TRY(load(dB, a.B, (size_t)batch * m));
    const double* vmin[] = {a.T, a.g, a.Y0, a.Y1, a.KY0, a.KY1, a.M, a.AX, a.optY, a.S0, a.S1, a.optS};
    double* vmdev[] = {dT, dg, dY[0], dY[1], dKY[0], dKY[1], dM, dAX, doptY, dS[0], dS[1], doptS};
    for (int k = 0; k < 12; ++k) ACE_TRY(load(vmdev[k], vmin[k], bm));
    const double* vnin[] = {a.Zb1, a.Zb2, a.Nb1, a.Nb2, a.X, a.Xcur, a.optX};
    double* vndev[] = {dZ[0], dZ[1], dN[0], dN[1], dX, dXcur, doptX};
    for (int k = 0; k < 7; ++k) ACE_TRY(load(vndev[k], vnin[k], bn));

    // admm_run's ZArgs block, then admm_iterate_split's per-iteration fields
    double* Zc = zodd ? dZ[0] : dZ[1];   // Z, N of the previous iterate (ping-pong)
    double* Nc = zodd ? dN[0] : dN[1];
    const unsigned char* r1 = a.rank_one ? dr1 : nullptr;
    const DualCtl dc{a.tol_abs, a.tol_rel, a.rho, a.fixed_iters, n, 1, ddone};
    ZArgs za{};
    za.n = n;
    za.m = m;
    za.r = 1;
    za.row_mode = 1;
    za.done_count = ddone;
    za.np = a.np;
    for (int p = 0; p < 4; ++p) za.fl[p] = a.fl[p];
    za.rank_one = r1;
    za.tol_rel = a.tol_rel;
    za.tol_abs = a.tol_abs;
    za.rho = a.rho;
    za.fixed_iters = a.fixed_iters;
    za.warm = 1;
    za.zeros = dzeros;
    za.lazy_dual = 1;
    za.Kf = L.K;
    za.it = it;
    za.wmode = 1;
    za.yfused = 1;
    za.X = dX;
    za.Z = Zc;
    za.N = Nc;
    za.Zn = zodd ? dZ[1] : dZ[0];
    za.Nn = zodd ? dN[1] : dN[0];
    za.st = drs;
    za.optX = doptX;
    za.optY = doptY;
    za.Xcur = dXcur;
    za.Ynew = dY[1 - q];
    za.Yold = dY[q];
    za.fixup_now = it == a.maxiter;
    za.lean = 1;
    za.xfuse = 1;
    za.msp = (gyf || msr) ? (msr ? 1 : a.msp != 0) : 0;
    za.Af = L.A;
    za.Sold = dS[(it + 1) & 1];
    za.Snew = dS[it & 1];
    za.optS = doptS;
    za.msp_fail_it = a.msp_fail_it;
    za.rccnt = ddone + 34;

    GykArgs ga{};
    ga.Gf = L.Gf;
    ga.T = dT;
    ga.B = dB;
    ga.Yo = dY[q];
    ga.M = dM;
    ga.Yn = dY[1 - q];
    ga.g = dg;
    ga.KYo = dKY[q];
    ga.KYn = dKY[1 - q];
    ga.optY = doptY;
    ga.LK = L.LK8;
    ga.c8 = L.c8;
    ga.rs = drs;
    ga.AX = ax ? dAX : nullptr;
    ga.yn_id = (gyk && a.yn_copy) ? 0 : 2 - q;
    ga.LA = la ? L.LA8 : nullptr;
    ga.Z = la ? Zc : nullptr;
    ga.N = la ? Nc : nullptr;
    ga.zeros = dzeros;
    ga.n = n;
    ga.lazy = lazy ? 1 : 0;
    ga.dc = dc;
    ga.glds = gyf ? 1 : 0;
    ga.msp = gyf && a.msp ? 1 : 0;
    ga.it = it;
    ga.Sold = za.Sold;
    ga.Snew = dS[it & 1];
    ga.optS = doptS;
    ga.np = a.np;
    for (int p = 0; p < 4; ++p) ga.fl[p] = a.fl[p];
    ga.rank_one = r1;
    ga.room = a.room;
    ga.recert = a.state_ext ? 1 : 0;

    switch (op) {
        case ACE_UNIT_GYK: launch_gyk(batch, m, ga, st); break;
        case ACE_UNIT_GYF: launch_gyf(batch, m, n, ga, L.LAH8, dX, za, a.ctl ? 1 : 0, st); break;
        case ACE_UNIT_AHF: launch_i8_apply_AH(batch, m, n, L.LAH8, dg, dX, L.c8, drs, st, &za); break;
        case ACE_UNIT_MSR: {
            const MsrArgs ma{L.Gf, dB, {dY[0], dY[1]}, dM, dAX, {dS[0], dS[1]}, doptS, doptY, drs, ddone + 8, ddone + 1,
                             ddone + 12, ddone + 40, batch, m, it, a.it_end};
            launch_msr(ma, za, a.waves, st);
            break;
        }
        case ACE_UNIT_READY: launch_msr_ready(batch, drs, it, ddone + 28, st); break;
        default:
            launch_i8_msp_optx(batch, m, n, L.LAH8, doptS, doptX, L.c8, drs, dZ[0], dZ[1], dS[0], dS[1], st);
            break;
    }
    ACE_LAUNCHED("ace_unit_host");
    ACE_HIP(hipDeviceSynchronize());

    ACE_TRY(d.get(a.B_out, dB, (size_t)batch * m + g));
    double* vmout[] = {a.T_out, a.g_out, a.Y0_out, a.Y1_out, a.KY0_out, a.KY1_out, a.M_out, a.AX_out, a.optY_out,
                       a.S0_out, a.S1_out, a.optS_out};
    for (int k = 0; k < 12; ++k) ACE_TRY(d.get(vmout[k], vmdev[k], bm + g));
    double* vnout[] = {a.Zb1_out, a.Zb2_out, a.Nb1_out, a.Nb2_out, a.X_out, a.Xcur_out, a.optX_out};
    for (int k = 0; k < 7; ++k) ACE_TRY(d.get(vnout[k], vndev[k], bn + g));
    ACE_TRY(d.get(rs.data(), drs, rs.size()));
    ACE_TRY(d.get(cnt, ddone, 64));
    for (int b = 0; b < batch; ++b) {
        const RealState& s = rs[b];
        if (a.state_out) {
            double* v = a.state_out + (size_t)b * nstate;
            if (a.state_ext) v[ACE_UNIT_NSTATE] = s.recert;
            v[0] = s.mu;
            v[1] = s.last_res;
            v[2] = s.opt_obj;
            v[3] = s.nB;
            v[4] = s.vbound;
            v[5] = s.obj2;
            v[6] = s.nAX2;
            v[7] = s.nY2;
            v[8] = s.nJM2;
            v[9] = s.dY2;
            v[10] = s.dAtY;
            v[11] = s.nAtY;
            for (int p = 0; p < 4; ++p) v[12 + p] = s.kf[p];
            v[16] = s.kfcum;
            v[17] = s.pd_dZ2;
            v[18] = s.pd_nZ2;
            v[19] = s.pd_rc;
            v[20] = s.fs0;
            v[21] = s.fs3;
        }
        if (a.flags_out) {
            int32_t* f = a.flags_out + (size_t)b * ACE_UNIT_NFLAG;
            f[0] = s.iters;
            f[1] = s.done;
            f[2] = s.status;
            f[3] = s.nzero;
            f[4] = s.avok;
            f[5] = s.optsrc;
            f[6] = s.optysrc;
            f[7] = s.kfok;
            f[8] = s.dpend;
            f[9] = s.fzit;
            f[10] = s.zit;
            f[11] = s.mzit;
            f[12] = s.msp;
            f[13] = s.z0id;
            f[14] = s.msp_pad;
            f[15] = s.mres;
        }
    }
    if (a.done_count_out) *a.done_count_out = cnt[0];
    if (a.mspcount_out) *a.mspcount_out = cnt[1];
    if (a.resume) *a.resume = cnt[8];
    if (a.steps)
        for (int k = 0; k < 4; ++k) a.steps[k] = cnt[12 + k];
    if (a.ready)
        for (int k = 0; k < 3; ++k) a.ready[k] = cnt[28 + k];
    if (a.vecw) *a.vecw = cnt[40];
    if (a.guard_ok) {
        // the guard block, every control-block field the entry does not carry (all zero on entry), and the counters
        // no launch here owns
        int ok = memcmp(&rs[batch], &rs_in[batch], sizeof(RealState)) == 0;
        for (int b = 0; b < batch && ok; ++b) {
            const RealState& s = rs[b];
            ok = s.objcol == 0 && (a.state_ext || s.recert == 0) && s.mres_pad_[0] == 0 && s.mres_pad_[1] == 0 && s.na == 0.0 &&
                 s.nbeta == 0.0 && s.nx0 == 0.0 && s.nopt_a == 0.0 && s.ncur_a == 0.0 && s.naz == 0.0 && s.nep2 == 0.0 &&
                 s.npad2_ == 0.0;
        }
        for (int k = 2; k < 64 && ok; ++k)
            if (k != 8 && !(k >= 12 && k < 16) && !(k >= 28 && k < 31) && k != 40) ok = cnt[k] == 0;   // ([34..35]: no Z-step here)
        *a.guard_ok = ok;
    }
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_unit_host(const ace_unit_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_unit_host: NULL arguments");
    return unit_run(*args);
}
