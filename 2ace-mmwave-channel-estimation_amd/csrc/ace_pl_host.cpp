// Test entry for the PhaseLift step kernels (ace_pl_host): host arrays in, one operation of ace_phaselift.hip,
// host arrays out.
//
// Nothing is re-implemented here.  Every operation calls the launcher the solve calls (launch_pl_*, launch_chol,
// launch_ztranspose, and the solve's own pl_apply_A / pl_g_y / pl_zasm for its GEMMs); PlArgs is filled the way
// solve_batch fills it (ace_phaselift_host.cpp) and one PlState per realisation is filled from the caller's state.
// Every device buffer starts from the caller's array, or from `sentinel` where there is none, and is followed by
// `guard` doubles (ints) of it.  After the launch every buffer comes back whole; a buffer the operation must not
// write, every guard, the rest of the eigensolver's scratch, the state's padding and one state block after the
// batch's are compared bit for bit with what was uploaded (guard_ok).
#include "ace_host.hpp"
#include "ace_phaselift.hpp"

namespace ace {
namespace {

enum Kind { KMAT, KVEC, KR, KRT, KBDM, KB, KLAM, KMISC, KMM, KBD };
// the f64 buffers, in the order of ace_pl_args
enum {
    bx, bxo, bz, bzo, by, bG, bZnew, bP, bVT, bV, bAx, bAxo, bAz, bAzo, bAy, bgAy, bgAx, bAex, bbvec, bR, bRT,
    bPg, bT, btau, bC, blam, bmisc, bK, bcholR, bV1, bw, NBUF
};
enum { iact, icnt, iok, iiters, istatus, NIBUF };
struct Buf {
    const char* name;
    const double* ace_pl_args::*in;
    double* ace_pl_args::*out;
    int kind;
};
struct IBuf {
    const char* name;
    const int32_t* ace_pl_args::*in;
    int32_t* ace_pl_args::*out;
};
#define PL_B(n, k) {#n, &ace_pl_args::n, &ace_pl_args::n##_out, k}
const Buf kBufs[NBUF] = {
    PL_B(x, KMAT),    PL_B(xo, KMAT),  PL_B(z, KMAT),   PL_B(zo, KMAT),   PL_B(y, KMAT),    PL_B(G, KMAT),
    PL_B(Znew, KMAT), PL_B(P, KMAT),   PL_B(VT, KMAT),  PL_B(V, KMAT),    PL_B(Ax, KVEC),   PL_B(Axo, KVEC),
    PL_B(Az, KVEC),   PL_B(Azo, KVEC), PL_B(Ay, KVEC),  PL_B(gAy, KVEC),  PL_B(gAx, KVEC),  PL_B(Aex, KVEC),
    PL_B(bvec, KVEC), PL_B(R, KR),     PL_B(RT, KRT),   PL_B(Pg, KBDM),   PL_B(T, KBDM),    PL_B(tau, KB),
    PL_B(C, KMAT),    PL_B(lam, KLAM), PL_B(misc, KMISC), PL_B(K, KMM),   PL_B(cholR, KMM), PL_B(V1, KBD),
    PL_B(w, KBD)};
#undef PL_B
#define PL_I(n) {#n, &ace_pl_args::n, &ace_pl_args::n##_out}
const IBuf kIBufs[NIBUF] = {PL_I(act), PL_I(cnt), PL_I(ok), PL_I(iters), PL_I(status)};
#undef PL_I

constexpr uint64_t M(int b) { return 1ull << b; }
struct Op {
    const char* name;
    uint64_t need, writes;      // f64 buffers that must be given / that the operation may write
    unsigned ineed, iwrites;    // the same for the int32 buffers
    bool need_state, writes_state;
};
const Op kOps[ACE_PL_NOPS] = {
    {"init", M(bbvec), M(bgAy) | M(bgAx), 0, 0, false, true},
    {"outer_begin", M(bx) | M(bz) | M(bAx) | M(bAz), M(bxo) | M(bzo) | M(bAxo) | M(bAzo), 0, 0, true, true},
    {"theta", 0, 0, 1u << icnt, 1u << iact | 1u << icnt, true, true},
    {"make_y", M(bxo) | M(bzo), M(by), 1u << iact, 0, true, false},
    {"set_ay", M(bAxo) | M(bAzo) | M(bAex), M(bAy), 1u << iact, 0, true, false},
    {"grad", M(bAy) | M(bbvec) | M(bgAy) | M(bR), M(bgAy) | M(bPg) | M(btau), 1u << iact, 0, true, true},
    {"gy", M(bR) | M(bPg), M(bG), 0, 0, false, false},
    {"prox_in", M(bzo) | M(bG), M(bC), 1u << iact, 0, true, false},
    {"assemble", M(bV) | M(blam) | M(bmisc) | M(btau), M(bP) | M(bVT), 1u << iact, 0, true, true},
    {"zasm", M(bVT) | M(bP) | M(bmisc), M(bZnew), 0, 0, false, false},
    {"take_z", M(bZnew) | M(bzo) | M(bG) | M(bmisc) | M(btau), M(bz), 1u << iact, 0, true, false},
    {"apply_a", M(bx) | M(bR) | M(bRT), M(bT) | M(bAex), 1u << iact, 0, false, false},
    {"make_x", M(bxo) | M(bz) | M(by) | M(bG) | M(bAxo) | M(bAz), M(bx) | M(bAx), 1u << iact | 1u << icnt, 1u << icnt,
     true, true},
    {"set_ax", M(bAex), M(bAx), 1u << iact, 0, true, false},
    {"backtrack", M(bAx) | M(bAy) | M(bbvec) | M(bgAy), M(bgAx), 1u << iact, 0, true, true},
    {"iterate", M(bx) | M(bAx) | M(bgAx), M(by) | M(bz) | M(bAy) | M(bAz) | M(bgAy), 1u << icnt, 1u << icnt, true, true},
    {"chol", M(bK), M(bcholR), 0, 1u << iok, false, false},
    {"transpose", M(bR), M(bRT), 0, 0, false, false},
    {"final_vec", M(bx) | M(bV1) | M(blam), M(bC) | M(bw), 0, 0, false, false},
    {"outputs", 0, 0, 0, 1u << iiters | 1u << istatus, true, false},
};

bool is_slot(int b) { return b == bC || b == blam || b == bmisc; }   // (live inside the eigensolver's scratch)

int pl_run(const ace_pl_args& a) {
    const int op = a.op, batch = a.batch, m = a.m, d = a.d;
    if (op < 0 || op >= ACE_PL_NOPS) return fail(ACE_ERR_ARG, "ace_pl_host: unknown op %d", op);
    const Op& o = kOps[op];
    const char* on = o.name;
    if (batch < 1 || batch > (1 << 16)) return fail(ACE_ERR_ARG, "ace_pl_host (%s): batch %d", on, batch);
    if (m < 1 || m > (1 << 16)) return fail(ACE_ERR_ARG, "ace_pl_host (%s): m %d", on, m);
    if (d < 1) return fail(ACE_ERR_ARG, "ace_pl_host (%s): d %d", on, d);
    if (d > 1600) return fail(ACE_ERR_UNSUPPORTED, "ace_pl_host (%s): d = %d > 1600 (eigensolver LDS limit)", on, d);
    if (a.guard < 0 || a.guard > (1 << 24)) return fail(ACE_ERR_ARG, "ace_pl_host (%s): guard %d", on, a.guard);
    const bool fin = op == ACE_PL_FINAL_VEC;
    if (fin && a.reduced && m != d)
        return fail(ACE_ERR_ARG, "ace_pl_host (%s): reduced needs m == d (got m %d, d %d)", on, m, d);
    for (int b = 0; b < NBUF; ++b)
        if (((o.need >> b) & 1) && !(a.*kBufs[b].in) && !(b == bR && fin && !a.reduced))
            return fail(ACE_ERR_ARG, "ace_pl_host (%s): NULL %s", on, kBufs[b].name);
    if (fin && a.reduced && !a.R) return fail(ACE_ERR_ARG, "ace_pl_host (%s): NULL R", on);
    for (int b = 0; b < NIBUF; ++b)
        if (((o.ineed >> b) & 1) && !(a.*kIBufs[b].in)) return fail(ACE_ERR_ARG, "ace_pl_host (%s): NULL %s", on, kIBufs[b].name);
    if (o.need_state && !a.state) return fail(ACE_ERR_ARG, "ace_pl_host (%s): NULL state", on);

    const size_t g = (size_t)a.guard, B = (size_t)batch, dd = (size_t)d * d;
    const HeevLayout hl = heev_layout(d, fin ? 1 : d);
    const size_t nscr = (size_t)hl.stride * B;
    size_t cnt[NBUF];
    for (int b = 0; b < NBUF; ++b) {
        switch (kBufs[b].kind) {
            case KMAT: cnt[b] = 2 * B * dd; break;
            case KVEC: cnt[b] = B * m; break;
            case KR:
            case KRT: cnt[b] = 2 * (size_t)d * m; break;
            case KBDM: cnt[b] = 2 * B * d * m; break;
            case KB: cnt[b] = B; break;
            case KLAM: cnt[b] = B * d; break;
            case KMISC: cnt[b] = 3 * B; break;
            case KMM: cnt[b] = 2 * (size_t)m * m; break;
            default: cnt[b] = 2 * B * d;
        }
    }
    const size_t icount[NIBUF] = {B, 9, 1, B, B};
    // the scratch slots the entry carries: [b][per] doubles at `off` of each realisation's stride
    const long long slot_off[3] = {hl.C, hl.lam, hl.misc};
    // (per: doubles carried of each host row of `row`; the final eig's layout keeps one eigenvalue, lam[b][0])
    const size_t slot_row[3] = {2 * dd, (size_t)d, 3};
    const size_t slot_per[3] = {2 * dd, fin ? (size_t)1 : (size_t)d, 3};
    const int slot_id[3] = {bC, blam, bmisc};
    for (int s = 0; s < 3; ++s)
        if (slot_off[s] < 0 || slot_off[s] + (long long)slot_per[s] > hl.stride)
            return fail(ACE_ERR_WORKSPACE, "ace_pl_host: the %s slot does not fit the eigensolver's layout", kBufs[slot_id[s]].name);

    double* dev[NBUF] = {};
    int32_t* idev[NIBUF] = {};
    double* dscr = nullptr;
    PlState* dst = nullptr;
    auto carve = [&](Carver& cv) {
        for (int b = 0; b < NBUF; ++b)
            if (!is_slot(b)) dev[b] = cv.take(8 * (cnt[b] + g));
        for (int b = 0; b < NIBUF; ++b) idev[b] = cv.take<int32_t>(4 * (icount[b] + g + 64));
        dscr = cv.take(8 * (nscr + g));
        dst = cv.take<PlState>(sizeof(PlState) * (B + 1));
    };
    DevScope dv;
    ACE_TRY(carve_zeroed(dv, carve));
    hipStream_t st = nullptr;

    // host images of what is uploaded
    std::vector<std::vector<double>> img(NBUF);
    std::vector<std::vector<int32_t>> iimg(NIBUF);
    std::vector<double> scr(nscr + g, a.sentinel);
    for (int b = 0; b < NBUF; ++b) {
        if (is_slot(b)) continue;
        img[b].assign(cnt[b] + g, a.sentinel);
        if (a.*kBufs[b].in) memcpy(img[b].data(), a.*kBufs[b].in, 8 * cnt[b]);
        ACE_TRY(dv.set(dev[b], img[b].data(), cnt[b] + g));
    }
    for (int s = 0; s < 3; ++s)
        if (const double* src = a.*kBufs[slot_id[s]].in)
            for (size_t b = 0; b < B; ++b)
                memcpy(&scr[b * hl.stride + slot_off[s]], src + b * slot_row[s], 8 * slot_per[s]);
    ACE_TRY(dv.set(dscr, scr.data(), nscr + g));
    for (int b = 0; b < NIBUF; ++b) {
        iimg[b].assign(icount[b] + g, (int32_t)ACE_PL_ISENTINEL);
        if (a.*kIBufs[b].in) memcpy(iimg[b].data(), a.*kIBufs[b].in, 4 * icount[b]);
        ACE_TRY(dv.set(idev[b], iimg[b].data(), icount[b] + g));
    }
    std::vector<PlState> ps(B + 1);
    memset(ps.data(), 0, sizeof(PlState) * ps.size());
    memset(&ps[B], 0x5A, sizeof(PlState));   // the guard block
    if (a.state)
        for (size_t b = 0; b < B; ++b) {
            const double* v = a.state + b * ACE_PL_NSTATE;
            PlState& p = ps[b];
            double* pd = &p.L;
            for (int i = 0; i < 16; ++i) pd[i] = v[i];
            int32_t* pi = &p.n_iter;
            for (int i = 0; i < 13; ++i) pi[i] = (int32_t)v[16 + i];
        }
    const std::vector<PlState> ps_in = ps;
    ACE_TRY(dv.set(dst, ps.data(), ps.size()));

    PlArgs pa{};
    pa.d = d;
    pa.m = m;
    pa.batch = batch;
    pa.cntr_reset = a.cntr_reset;
    pa.restart = a.restart;
    pa.maxIts = a.maxIts;
    pa.lambda = a.lambda;
    pa.alpha = a.alpha;
    pa.beta = a.beta;
    pa.Lexact = a.Lexact;
    pa.tol = a.tol;
    pa.L0 = a.L0;
    pa.x = dev[bx], pa.xo = dev[bxo], pa.z = dev[bz], pa.zo = dev[bzo], pa.y = dev[by], pa.G = dev[bG];
    pa.Znew = dev[bZnew], pa.P = dev[bP], pa.VT = dev[bVT], pa.V = dev[bV];
    pa.Ax = dev[bAx], pa.Axo = dev[bAxo], pa.Az = dev[bAz], pa.Azo = dev[bAzo], pa.Ay = dev[bAy];
    pa.gAy = dev[bgAy], pa.gAx = dev[bgAx], pa.Aex = dev[bAex];
    pa.bvec = dev[bbvec];
    pa.R = dev[bR];
    pa.Pg = dev[bPg];
    pa.st = dst;
    pa.act = idev[iact];
    pa.cnt = idev[icnt];
    pa.scratch = dscr;
    pa.hl = hl;
    pa.tau = dev[btau];

    switch (op) {
        case ACE_PL_INIT: launch_pl_init(pa, st); break;
        case ACE_PL_OUTER_BEGIN: launch_pl_outer_begin(pa, st); break;
        case ACE_PL_THETA: launch_pl_theta(pa, st); break;
        case ACE_PL_MAKE_Y: launch_pl_make_y(pa, st); break;
        case ACE_PL_SET_AY: launch_pl_set_Ay(pa, st); break;
        case ACE_PL_GRAD: launch_pl_grad(pa, st); break;
        case ACE_PL_GY: pl_g_y(pa, st); break;
        case ACE_PL_PROX_IN: launch_pl_prox_in(pa, st); break;
        case ACE_PL_ASSEMBLE: launch_pl_assemble(pa, st); break;
        case ACE_PL_ZASM: pl_zasm(pa, st); break;
        case ACE_PL_TAKE_Z: launch_pl_take_z(pa, st); break;
        case ACE_PL_APPLY_A: pl_apply_A(pa, dev[bRT], dev[bT], pa.x, pa.Aex, st); break;
        case ACE_PL_MAKE_X: launch_pl_make_x(pa, st); break;
        case ACE_PL_SET_AX: launch_pl_set_Ax(pa, st); break;
        case ACE_PL_BACKTRACK: launch_pl_backtrack(pa, st); break;
        case ACE_PL_ITERATE: launch_pl_iterate(pa, st); break;
        case ACE_PL_CHOL: launch_chol(m, dev[bK], dev[bcholR], idev[iok], st); break;
        case ACE_PL_TRANSPOSE: launch_ztranspose(d, m, dev[bR], dev[bRT], st); break;
        case ACE_PL_FINAL_VEC:
            launch_pl_final_in(d, batch, pa.x, dscr, hl, st);
            launch_pl_final_vec(d, batch, a.reduced != 0, pa.R, dev[bV1], dscr, hl, dev[bw], st);
            break;
        default: launch_pl_outputs(batch, dst, idev[iiters], (uint32_t*)idev[istatus], st);
    }
    ACE_LAUNCHED("ace_pl_host");
    ACE_HIP(hipDeviceSynchronize());

    int ok = 1;
    std::vector<double> now;
    for (int b = 0; b < NBUF; ++b) {
        if (is_slot(b)) continue;
        now.resize(cnt[b] + g);
        ACE_TRY(dv.get(now.data(), dev[b], cnt[b] + g));
        const bool wr = (o.writes >> b) & 1;
        if (memcmp(now.data() + (wr ? cnt[b] : 0), img[b].data() + (wr ? cnt[b] : 0), 8 * (wr ? g : cnt[b] + g))) ok = 0;
        if (double* out = a.*kBufs[b].out) memcpy(out, now.data(), 8 * (cnt[b] + g));
    }
    now.resize(nscr + g);
    ACE_TRY(dv.get(now.data(), dscr, nscr + g));
    for (int s = 0; s < 3; ++s) {
        double* out = a.*kBufs[slot_id[s]].out;
        const double* in = a.*kBufs[slot_id[s]].in;
        const bool wr = (o.writes >> slot_id[s]) & 1;
        for (size_t b = 0; b < B; ++b) {
            double* at = &now[b * hl.stride + slot_off[s]];
            if (out) {
                for (size_t e = 0; e < slot_row[s]; ++e)   // (what the layout does not hold: as it came in)
                    out[b * slot_row[s] + e] = e < slot_per[s] ? at[e] : (in ? in[b * slot_row[s] + e] : a.sentinel);
            }
            if (wr) memcpy(&scr[b * hl.stride + slot_off[s]], at, 8 * slot_per[s]);   // (excluded from the comparison)
        }
        if (out) memcpy(out + B * slot_row[s], &now[nscr], 8 * g);
    }
    if (memcmp(now.data(), scr.data(), 8 * (nscr + g))) ok = 0;
    std::vector<int32_t> inow;
    for (int b = 0; b < NIBUF; ++b) {
        inow.resize(icount[b] + g);
        ACE_TRY(dv.get(inow.data(), idev[b], icount[b] + g));
        const bool wr = (o.iwrites >> b) & 1;
        if (memcmp(inow.data() + (wr ? icount[b] : 0), iimg[b].data() + (wr ? icount[b] : 0),
                   4 * (wr ? g : icount[b] + g)))
            ok = 0;
        if (int32_t* out = a.*kIBufs[b].out) memcpy(out, inow.data(), 4 * (icount[b] + g));
    }
    ACE_TRY(dv.get(ps.data(), dst, ps.size()));
    if (memcmp(&ps[B], &ps_in[B], sizeof(PlState))) ok = 0;
    for (size_t b = 0; b < B; ++b) {
        const PlState& p = ps[b];
        if (o.writes_state ? memcmp(p.pad, ps_in[b].pad, sizeof p.pad) : memcmp(&p, &ps_in[b], sizeof p)) ok = 0;
        if (a.state_out) {
            double* v = a.state_out + b * ACE_PL_NSTATE;
            const double* pd = &p.L;
            for (int i = 0; i < 16; ++i) v[i] = pd[i];
            const int32_t* pi = &p.n_iter;
            for (int i = 0; i < 13; ++i) v[16 + i] = (double)pi[i];
        }
    }
    if (a.guard_ok) *a.guard_ok = ok;
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

static_assert(sizeof(PlState) == 16 * 8 + 16 * 4, "ace_pl_host carries PlState as 16 doubles and 13 of its 16 ints");
static_assert(ACE_PL_NSTATE == 29, "PlState's carried fields");

extern "C" int ace_pl_host(const ace_pl_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_pl_host: NULL arguments");
    return pl_run(*args);
}
