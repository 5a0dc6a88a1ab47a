// Test entry for the kernels of the r-column stages and of the pipeline around them (ace_stage_host):
// host arrays in, one call of the pipeline's own launcher (ace_stage.hip), host arrays out.
//
// Nothing is re-implemented here.  Each op uploads its operands, fills the output buffers with the
// caller's sentinel, fills one RealState per realisation from `state` / `flags` (every other field
// zero) where the kernel reads one, and makes the one launcher call ace_admm.cpp / ace_pipeline.cpp
// make.  Every argument is checked before the first HIP call: sizes, NULL arrays, and every index
// table a kernel would follow (rows must be a permutation of 0 .. m-1 per realisation, idx within the
// destination), so that no argument of this entry can send a kernel out of bounds.
#include <algorithm>

#include "ace_host.hpp"
#include "ace_pipe.hpp"

namespace ace {
namespace {

const char* const kOpName[ACE_STAGE_NOPS] = {
    "init_r",      "ystep_r",      "finalize_r", "gram_rotate", "quality",     "part_quality", "keep_best",
    "finish",      "part_geinv",   "part_gfix",  "part_expand", "part_compact", "anorm",       "bnorm",
    "gather_rows", "gather_b",     "move_rows",  "move_bytes",  "put_col",     "flag_bits",    "fill"};

#define SG_NEED(field)                                                                                  \
    do {                                                                                                \
        if (!a.field) return fail(ACE_ERR_ARG, "ace_stage_host(%s): NULL %s", kOpName[a.op], #field);   \
    } while (0)
#define SG_RANGE(field, lo, hi)                                                                         \
    do {                                                                                                \
        if ((long long)a.field < (long long)(lo) || (long long)a.field > (long long)(hi))               \
            return fail(ACE_ERR_ARG, "ace_stage_host(%s): %s = %lld outside [%lld, %lld]", kOpName[a.op], \
                        #field, (long long)a.field, (long long)(lo), (long long)(hi));                  \
    } while (0)

constexpr int SG_MAXDIM = 4096, SG_MAXBATCH = 4096;

// rows [batch][m]: a permutation of 0 .. m-1 per realisation (train rows, then the test rows)
int check_rows(const ace_stage_args& a) {
    std::vector<unsigned char> seen((size_t)a.m);
    for (int b = 0; b < a.batch; ++b) {
        std::fill(seen.begin(), seen.end(), 0);
        for (int i = 0; i < a.m; ++i) {
            const int v = a.rows[(size_t)b * a.m + i];
            if (v < 0 || v >= a.m || seen[v])
                return fail(ACE_ERR_ARG, "ace_stage_host(%s): rows of realisation %d are no permutation of 0 .. m-1",
                            kOpName[a.op], b);
            seen[v] = 1;
        }
    }
    return ACE_OK;
}
int check_idx(const ace_stage_args& a, int count, int limit, bool distinct) {
    std::vector<unsigned char> seen((size_t)limit);
    for (int k = 0; k < count; ++k) {
        const int v = a.idx[k];
        if (v < 0 || v >= limit || (distinct && seen[v]))
            return fail(ACE_ERR_ARG, "ace_stage_host(%s): idx[%d] = %d outside [0, %d) or repeated", kOpName[a.op], k, v,
                        limit);
        seen[v] = 1;
    }
    return ACE_OK;
}
// the partition sizes: ACE_ERR_UNSUPPORTED past the test rows the per-realisation kernels take
int check_part(const ace_stage_args& a) {
    SG_RANGE(m, 1, SG_MAXDIM);
    SG_RANGE(mt, 1, a.m);
    if (a.m - a.mt > PART_MAXTE)
        return fail(ACE_ERR_UNSUPPORTED, "ace_stage_host(%s): m - mt = %d test rows, the kernels take %d", kOpName[a.op],
                    a.m - a.mt, PART_MAXTE);
    SG_NEED(rows);
    return check_rows(a);
}
int check_r(const ace_stage_args& a) {
    if (a.r > 32) return fail(ACE_ERR_UNSUPPORTED, "ace_stage_host(%s): r = %d, the kernels take 32", kOpName[a.op], a.r);
    SG_RANGE(r, 1, 32);
    return ACE_OK;
}

void fill_state(const ace_stage_args& a, std::vector<RealState>& rs) {
    memset(rs.data(), 0, sizeof(RealState) * rs.size());
    for (int b = 0; b < a.batch; ++b) {
        RealState& s = rs[b];
        s.mu = 1.0;
        if (a.state) {
            const double* v = a.state + (size_t)b * ACE_SG_NSTATE;
            s.mu = v[0];
            s.last_res = v[1];
            s.opt_obj = v[2];
            s.nB = v[3];
            s.obj2 = v[4];
            s.nAX2 = v[5];
            s.nY2 = v[6];
            s.nJM2 = v[7];
            s.dY2 = v[8];
        }
        if (a.flags) {
            const int32_t* f = a.flags + (size_t)b * ACE_SG_NFLAG;
            s.iters = f[0];
            s.done = f[1];
            s.status = f[2];
            s.objcol = f[3];
            s.optsrc = f[4];
            s.optysrc = f[5];
        }
    }
}
void read_state(const ace_stage_args& a, const std::vector<RealState>& rs) {
    for (int b = 0; b < a.batch; ++b) {
        const RealState& s = rs[b];
        if (a.state_out) {
            double* v = a.state_out + (size_t)b * ACE_SG_NSTATE;
            v[0] = s.mu;
            v[1] = s.last_res;
            v[2] = s.opt_obj;
            v[3] = s.nB;
            v[4] = s.obj2;
            v[5] = s.nAX2;
            v[6] = s.nY2;
            v[7] = s.nJM2;
            v[8] = s.dY2;
        }
        if (a.flags_out) {
            int32_t* f = a.flags_out + (size_t)b * ACE_SG_NFLAG;
            f[0] = s.iters;
            f[1] = s.done;
            f[2] = s.status;
            f[3] = s.objcol;
            f[4] = s.optsrc;
            f[5] = s.optysrc;
        }
    }
}

int stage_run(const ace_stage_args& a) {
    if (a.op < 0 || a.op >= ACE_STAGE_NOPS) return fail(ACE_ERR_ARG, "ace_stage_host: unknown op %d", a.op);
    const size_t batch = (size_t)a.batch, n = (size_t)a.n, m = (size_t)a.m, r = (size_t)a.r;
    const double sv = a.sentinel;
    const int32_t si = a.isentinel;
    DevScope d;
    hipStream_t st = nullptr;
    std::vector<RealState> rs;
    RealState* drs = nullptr;
    auto state_up = [&]() -> int {
        rs.resize(batch);
        fill_state(a, rs);
        return d.put(&drs, rs.data(), batch, RealState{});
    };
    auto state_down = [&]() -> int {
        ACE_TRY(d.get(rs.data(), drs, batch));
        read_state(a, rs);
        return ACE_OK;
    };
    auto launched = [&]() -> int {
        ACE_LAUNCHED("ace_stage_host");
        ACE_HIP(hipDeviceSynchronize());
        return ACE_OK;
    };

    switch (a.op) {
    case ACE_STAGE_INIT_R:
    case ACE_STAGE_YSTEP_R: {
        const bool init = a.op == ACE_STAGE_INIT_R;
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(m, 1, SG_MAXDIM);
        ACE_TRY(check_r(a));
        if (init) {
            SG_RANGE(n, 1, SG_MAXDIM);
            SG_NEED(X);
            SG_NEED(P0);
            if (!(a.mu0 > 0.0)) return fail(ACE_ERR_ARG, "ace_stage_host(init_r): mu0 = %g", a.mu0);
        } else {
            SG_NEED(S);
            SG_NEED(g);
            SG_NEED(M);
            SG_NEED(Y);
        }
        SG_NEED(B);
        const size_t bn = 2 * batch * r * n, bm = 2 * batch * r * m;
        unsigned char* dmask = nullptr;
        if (a.mask) ACE_TRY(d.put(&dmask, a.mask, batch * m, 0));
        const PartRows pr{nullptr, dmask, nullptr, a.m, a.m, a.m};
        double *dB, *dYo, *dM;
        ACE_TRY(d.put(&dB, a.B, batch * m, 0.0));
        ACE_TRY(d.put(&dYo, nullptr, bm, sv));
        ACE_TRY(state_up());
        if (init) {
            double *dX0, *dP0, *dXo, *dNo;
            ACE_TRY(d.put(&dX0, a.X, bn, 0.0));
            ACE_TRY(d.put(&dP0, a.P0, bm, 0.0));
            ACE_TRY(d.put(&dXo, nullptr, bn, sv));
            ACE_TRY(d.put(&dNo, nullptr, bn, sv));
            ACE_TRY(d.put(&dM, nullptr, bm, sv));
            launch_init_r(a.row_mode, a.n, a.m, a.r, a.batch, dX0, dP0, dB, dXo, dYo, dM, dNo, drs, a.mu0, st,
                          a.mask ? &pr : nullptr);
            ACE_TRY(launched());
            ACE_TRY(d.get(a.Xo, dXo, bn));
            ACE_TRY(d.get(a.No, dNo, bn));
        } else {
            double *dS, *dg, *dYold;
            ACE_TRY(d.put(&dS, a.S, bm, 0.0));
            ACE_TRY(d.put(&dg, a.g, bm, 0.0));
            ACE_TRY(d.put(&dM, a.M, bm, 0.0));
            ACE_TRY(d.put(&dYold, a.Y, bm, 0.0));
            launch_ystep_r(a.row_mode, a.m, a.r, a.batch, dS, dg, dM, dB, dYold, dYo, drs, st, a.mask ? &pr : nullptr);
            ACE_TRY(launched());
        }
        ACE_TRY(d.get(a.Yo, dYo, bm));
        ACE_TRY(d.get(a.Mo, dM, bm));
        return state_down();
    }
    case ACE_STAGE_FINALIZE_R: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(n, 1, SG_MAXDIM);
        SG_RANGE(m, 1, SG_MAXDIM);
        ACE_TRY(check_r(a));
        SG_RANGE(nc, 1, a.r);
        SG_NEED(optX);
        SG_NEED(optY);
        SG_NEED(X);
        SG_NEED(Y);
        const size_t nc = (size_t)a.nc, on = 2 * batch * nc * n, om = 2 * batch * nc * m;
        double *doX, *doY, *dX, *dY, *dXo, *dYo, *dmu, *dz1 = nullptr, *dz2 = nullptr, *dy1 = nullptr, *dy2 = nullptr;
        int32_t* dit;
        uint32_t* dst;
        ACE_TRY(d.put(&doX, a.optX, on, 0.0));
        ACE_TRY(d.put(&doY, a.optY, om, 0.0));
        ACE_TRY(d.put(&dX, a.X, 2 * batch * r * n, 0.0));
        ACE_TRY(d.put(&dY, a.Y, 2 * batch * r * m, 0.0));
        if (a.Zb1) ACE_TRY(d.put(&dz1, a.Zb1, on, 0.0));
        if (a.Zb2) ACE_TRY(d.put(&dz2, a.Zb2, on, 0.0));
        if (a.Yb1) ACE_TRY(d.put(&dy1, a.Yb1, om, 0.0));
        if (a.Yb2) ACE_TRY(d.put(&dy2, a.Yb2, om, 0.0));
        ACE_TRY(d.put(&dXo, nullptr, on, sv));
        ACE_TRY(d.put(&dYo, nullptr, om, sv));
        ACE_TRY(d.put(&dmu, nullptr, batch, sv));
        ACE_TRY(d.put(&dit, nullptr, batch, si));
        ACE_TRY(d.put(&dst, nullptr, batch, (uint32_t)si));
        ACE_TRY(state_up());
        launch_finalize_r(a.n, a.m, a.r, a.nc, a.batch, doX, doY, dX, dY, dXo, dYo, dit, dst, dmu, drs, st, dz1, dz2, dy1,
                          dy2);
        ACE_TRY(launched());
        ACE_TRY(d.get(a.Xo, dXo, on));
        ACE_TRY(d.get(a.Yo, dYo, om));
        ACE_TRY(d.get(a.qo, dmu, batch));
        if (a.iout) {   // [batch][2]: iters, status
            std::vector<int32_t> it(batch), sb(batch);
            ACE_TRY(d.get(it.data(), dit, batch));
            ACE_TRY(d.get(reinterpret_cast<uint32_t*>(sb.data()), dst, batch));
            for (size_t b = 0; b < batch; ++b) {
                a.iout[2 * b] = it[b];
                a.iout[2 * b + 1] = sb[b];
            }
        }
        return ACE_OK;
    }
    case ACE_STAGE_GRAM_ROTATE: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(n, 1, SG_MAXDIM);
        ACE_TRY(check_r(a));
        SG_NEED(X);
        double* dX;
        int* dstat;
        ACE_TRY(d.put(&dX, a.X, 2 * batch * r * n, 0.0));
        ACE_TRY(d.put(&dstat, a.idst, batch, 0));
        launch_gram_rotate(a.n, a.r, a.batch, dX, dstat, st);
        ACE_TRY(launched());
        ACE_TRY(d.get(a.Xo, dX, 2 * batch * r * n));
        return d.get(a.iout, dstat, batch);
    }
    case ACE_STAGE_QUALITY:
    case ACE_STAGE_PART_QUALITY: {
        const bool part = a.op == ACE_STAGE_PART_QUALITY;
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(n, 1, SG_MAXDIM);
        if (part) ACE_TRY(check_part(a));
        else SG_RANGE(count, 0, SG_MAXDIM);
        SG_NEED(X);
        if (part || a.count > 0) {
            SG_NEED(A);
            SG_NEED(B);
        }
        const size_t rowsA = part ? m : (size_t)a.count;
        double *dA, *dX, *dB, *dq;
        ACE_TRY(d.put(&dA, a.A, 2 * rowsA * n, 0.0));
        ACE_TRY(d.put(&dX, a.X, 2 * batch * n, 0.0));
        ACE_TRY(d.put(&dB, a.B, batch * rowsA, 0.0));
        ACE_TRY(d.put(&dq, nullptr, batch, sv));
        if (part) {
            int* drows;
            ACE_TRY(d.put(&drows, a.rows, batch * m, 0));
            const PartRows pr{drows, nullptr, nullptr, a.m, a.mt, a.m};
            launch_part_quality(a.n, a.batch, pr, dA, dX, dB, dq, st);
        } else {
            launch_quality(a.n, a.count, a.batch, dA, dX, dB, dq, st);
        }
        ACE_TRY(launched());
        return d.get(a.qo, dq, batch);
    }
    case ACE_STAGE_KEEP_BEST: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(n, 1, SG_MAXDIM);
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_NEED(q);
        SG_NEED(qmax);
        SG_NEED(X);
        SG_NEED(Y);
        double *dq, *dqm, *dX, *dY, *dXm, *dYm;
        ACE_TRY(d.put(&dq, a.q, batch, 0.0));
        ACE_TRY(d.put(&dqm, a.qmax, batch, 0.0));
        ACE_TRY(d.put(&dX, a.X, 2 * batch * n, 0.0));
        ACE_TRY(d.put(&dY, a.Y, 2 * batch * m, 0.0));
        ACE_TRY(d.put(&dXm, a.Xmax, 2 * batch * n, sv));
        ACE_TRY(d.put(&dYm, a.Ymax, 2 * batch * m, sv));
        launch_keep_best(a.n, a.m, a.batch, a.first != 0, dq, dqm, dX, dY, dXm, dYm, st);
        ACE_TRY(launched());
        ACE_TRY(d.get(a.qo, dqm, batch));
        ACE_TRY(d.get(a.Xo, dXm, 2 * batch * n));
        return d.get(a.Yo, dYm, 2 * batch * m);
    }
    case ACE_STAGE_FINISH: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(n, 1, SG_MAXDIM);
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(mt, 1, a.m);
        SG_NEED(q);
        SG_NEED(X);
        SG_NEED(Y);
        SG_NEED(Xmax);
        SG_NEED(Ymax);
        SG_NEED(anorm);
        SG_NEED(bnorm);
        double *dq, *dX, *dY, *dXm, *dYm, *dan, *dbn, *dXo, *dYo;
        uint32_t* dstat;
        ACE_TRY(d.put(&dq, a.q, batch, 0.0));
        ACE_TRY(d.put(&dX, a.X, 2 * batch * n, 0.0));
        ACE_TRY(d.put(&dY, a.Y, 2 * batch * m, 0.0));
        ACE_TRY(d.put(&dXm, a.Xmax, 2 * batch * n, 0.0));
        ACE_TRY(d.put(&dYm, a.Ymax, 2 * batch * (size_t)a.mt, 0.0));
        ACE_TRY(d.put(&dan, a.anorm, 1, 0.0));
        ACE_TRY(d.put(&dbn, a.bnorm, batch, 0.0));
        ACE_TRY(d.put(&dXo, nullptr, 2 * batch * n, sv));
        ACE_TRY(d.put(&dYo, nullptr, 2 * batch * m, sv));
        ACE_TRY(d.put(&dstat, reinterpret_cast<const uint32_t*>(a.idst), batch, 0u));
        launch_finish(a.n, a.m, a.mt, a.batch, dq, dX, dY, dXm, dYm, dan, dbn, dXo, dYo, dstat, st);
        ACE_TRY(launched());
        ACE_TRY(d.get(a.Xo, dXo, 2 * batch * n));
        ACE_TRY(d.get(a.Yo, dYo, 2 * batch * m));
        return d.get(reinterpret_cast<uint32_t*>(a.iout), dstat, batch);
    }
    case ACE_STAGE_PART_GEINV:
    case ACE_STAGE_PART_GFIX: {
        const bool fix = a.op == ACE_STAGE_PART_GFIX;
        SG_RANGE(batch, 1, SG_MAXBATCH);
        ACE_TRY(check_part(a));
        SG_NEED(G);
        const size_t te = (size_t)(a.m - a.mt);
        if (fix) {
            ACE_TRY(check_r(a));
            SG_NEED(g);
            SG_NEED(mask);
            if (te) SG_NEED(geinv);
            for (int b = 0; b < a.batch; ++b)   // the mask is the partition's: 1 on rows[:mt], 0 on rows[mt:]
                for (int i = 0; i < a.m; ++i)
                    if ((a.mask[(size_t)b * m + a.rows[(size_t)b * m + i]] != 0) != (i < a.mt))
                        return fail(ACE_ERR_ARG, "ace_stage_host(part_gfix): mask of realisation %d differs from rows", b);
        }
        double *dG, *dgi;
        int* drows;
        ACE_TRY(d.put(&dG, a.G, 2 * m * m, 0.0));
        ACE_TRY(d.put(&drows, a.rows, batch * m, 0));
        if (!fix) {
            int* dstat;
            ACE_TRY(d.put(&dgi, nullptr, 2 * batch * te * te, sv));
            ACE_TRY(d.put(&dstat, a.idst, batch, 0));
            const PartRows pr{drows, nullptr, dgi, a.m, a.mt, a.m};
            launch_part_geinv(a.batch, pr, dG, dgi, dstat, st);
            ACE_TRY(launched());
            ACE_TRY(d.get(a.Xo, dgi, 2 * batch * te * te));
            return d.get(a.iout, dstat, batch);
        }
        unsigned char* dmask;
        double* dg;
        ACE_TRY(d.put(&dgi, a.geinv, 2 * batch * te * te, 0.0));
        ACE_TRY(d.put(&dmask, a.mask, batch * m, 0));
        ACE_TRY(d.put(&dg, a.g, 2 * batch * r * m, 0.0));
        if (a.flags) ACE_TRY(state_up());
        const PartRows pr{drows, dmask, dgi, a.m, a.mt, a.m};
        launch_part_gfix(a.batch, a.r, pr, dG, dg, a.flags ? drs : nullptr, st);
        ACE_TRY(launched());
        return d.get(a.Yo, dg, 2 * batch * r * m);
    }
    case ACE_STAGE_PART_EXPAND:
    case ACE_STAGE_PART_COMPACT: {
        const bool expand = a.op == ACE_STAGE_PART_EXPAND;
        SG_RANGE(batch, 1, SG_MAXBATCH);
        ACE_TRY(check_part(a));
        ACE_TRY(check_r(a));
        SG_NEED(Y);
        const size_t cm = 2 * batch * r * (size_t)a.mt, fm = 2 * batch * r * m;
        double *dsrc, *ddst;
        int* drows;
        ACE_TRY(d.put(&drows, a.rows, batch * m, 0));
        ACE_TRY(d.put(&dsrc, a.Y, expand ? cm : fm, 0.0));
        ACE_TRY(d.put(&ddst, nullptr, expand ? fm : cm, sv));
        const PartRows pr{drows, nullptr, nullptr, a.m, a.mt, a.m};
        if (expand) launch_part_expand(a.batch, a.r, pr, dsrc, ddst, st);
        else launch_part_compact(a.batch, a.r, pr, dsrc, ddst, st);
        ACE_TRY(launched());
        return d.get(a.Yo, ddst, expand ? fm : cm);
    }
    case ACE_STAGE_ANORM: {
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(n, 1, SG_MAXDIM);
        SG_NEED(A);
        double *dA, *dq;
        ACE_TRY(d.put(&dA, a.A, 2 * m * n, 0.0));
        ACE_TRY(d.put(&dq, nullptr, 1, sv));
        launch_anorm(a.m, a.n, dA, a.tol_abs, dq, st);
        ACE_TRY(launched());
        return d.get(a.qo, dq, 1);
    }
    case ACE_STAGE_BNORM: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_NEED(B);
        double *dB, *dq, *dBn;
        ACE_TRY(d.put(&dB, a.B, batch * m, 0.0));
        ACE_TRY(d.put(&dq, nullptr, batch, sv));
        ACE_TRY(d.put(&dBn, nullptr, batch * m, sv));
        launch_bnorm(a.m, a.batch, dB, a.tol_abs, dq, dBn, st);
        ACE_TRY(launched());
        ACE_TRY(d.get(a.qo, dq, batch));
        return d.get(a.Xo, dBn, batch * m);
    }
    case ACE_STAGE_GATHER_ROWS: {
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(n, 1, SG_MAXDIM);
        SG_RANGE(count, 0, SG_MAXDIM);
        SG_NEED(A);
        SG_NEED(anorm);
        if (a.count) SG_NEED(idx);
        ACE_TRY(check_idx(a, a.count, a.m, false));
        double *dA, *dan, *dd;
        int* didx;
        ACE_TRY(d.put(&dA, a.A, 2 * m * n, 0.0));
        ACE_TRY(d.put(&dan, a.anorm, 1, 0.0));
        ACE_TRY(d.put(&didx, a.idx, (size_t)a.count, 0));
        ACE_TRY(d.put(&dd, nullptr, 2 * (size_t)a.count * n, sv));
        launch_gather_rows(a.count, a.n, dA, didx, dan, dd, st);
        ACE_TRY(launched());
        return d.get(a.Xo, dd, 2 * (size_t)a.count * n);
    }
    case ACE_STAGE_GATHER_B: {
        SG_RANGE(batch, 1, SG_MAXBATCH);
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(count, 0, SG_MAXDIM);
        SG_NEED(B);
        if (a.count) SG_NEED(idx);
        ACE_TRY(check_idx(a, a.count, a.m, false));
        double *dB, *dd;
        int* didx;
        ACE_TRY(d.put(&dB, a.B, batch * m, 0.0));
        ACE_TRY(d.put(&didx, a.idx, (size_t)a.count, 0));
        ACE_TRY(d.put(&dd, nullptr, batch * (size_t)a.count, sv));
        launch_gather_b(a.m, a.count, a.batch, dB, didx, dd, st);
        ACE_TRY(launched());
        return d.get(a.qo, dd, batch * (size_t)a.count);
    }
    case ACE_STAGE_MOVE_ROWS:
    case ACE_STAGE_MOVE_BYTES: {
        // count moved rows of len doubles / bytes; the other side has m rows (gather: the source; scatter: the
        // destination, whose idx are distinct)
        const bool bytes = a.op == ACE_STAGE_MOVE_BYTES, sc = a.scatter != 0;
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(count, 0, SG_MAXDIM);
        SG_RANGE(len, 1, 1 << 20);
        if (a.count) SG_NEED(idx);
        if (bytes) SG_NEED(bsrc);
        else SG_NEED(src);
        ACE_TRY(check_idx(a, a.count, a.m, sc));
        const size_t len = (size_t)a.len, ns = (sc ? (size_t)a.count : m) * len, nd = (sc ? m : (size_t)a.count) * len;
        int* didx;
        ACE_TRY(d.put(&didx, a.idx, (size_t)a.count, 0));
        if (bytes) {
            unsigned char *ds, *dd;
            ACE_TRY(d.put(&ds, a.bsrc, ns, 0));
            ACE_TRY(d.put(&dd, nullptr, nd, (unsigned char)si));
            launch_move_bytes(a.count, a.len, ds, dd, didx, sc, st);
            ACE_TRY(launched());
            return d.get(a.bout, dd, nd);
        }
        double *ds, *dd;
        ACE_TRY(d.put(&ds, a.src, ns, 0.0));
        ACE_TRY(d.put(&dd, nullptr, nd, sv));
        launch_move_rows(a.count, a.len, ds, dd, didx, sc, st);
        ACE_TRY(launched());
        return d.get(a.qo, dd, nd);
    }
    case ACE_STAGE_PUT_COL: {
        // dst [m][ld] int32 (idst, or isentinel), count <= (idx ? any : m) sources
        SG_RANGE(m, 1, SG_MAXDIM);
        SG_RANGE(ld, 1, 64);
        SG_RANGE(col, 0, a.ld - 1);
        SG_RANGE(count, 0, a.idx ? SG_MAXDIM : a.m);
        if (a.count) SG_NEED(isrc);
        if (a.idx) ACE_TRY(check_idx(a, a.count, a.m, true));
        int *ds, *didx = nullptr, *dd;
        ACE_TRY(d.put(&ds, a.isrc, (size_t)a.count, 0));
        if (a.idx) ACE_TRY(d.put(&didx, a.idx, (size_t)a.count, 0));
        ACE_TRY(d.put(&dd, a.idst, m * (size_t)a.ld, si));
        launch_put_col(a.count, ds, didx, dd, a.ld, a.col, a.or_mask, st);
        ACE_TRY(launched());
        return d.get(a.iout, dd, m * (size_t)a.ld);
    }
    case ACE_STAGE_FLAG_BITS: {
        // dst [m] int32 (idst, or isentinel), flag [count], count <= m
        SG_RANGE(m, 1, 1 << 20);
        SG_RANGE(count, 0, a.m);
        if (a.count) SG_NEED(bsrc);
        unsigned char* df;
        int* dd;
        ACE_TRY(d.put(&df, a.bsrc, (size_t)a.count, 0));
        ACE_TRY(d.put(&dd, a.idst, m, si));
        launch_flag_bits(a.count, df, dd, a.bit, st);
        ACE_TRY(launched());
        return d.get(a.iout, dd, m);
    }
    case ACE_STAGE_FILL: {
        // dst [m] doubles of sentinel, the first len set to value
        SG_RANGE(m, 1, 1 << 24);
        SG_RANGE(len, 0, a.m);
        double* dd;
        ACE_TRY(d.put(&dd, nullptr, m, sv));
        launch_fill(a.len, a.value, dd, st);
        ACE_TRY(launched());
        return d.get(a.qo, dd, m);
    }
    }
    return fail(ACE_ERR_ARG, "ace_stage_host: unknown op %d", a.op);
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_stage_host(const ace_stage_args* args) {
    g_err.clear();
    if (!args) return fail(ACE_ERR_ARG, "ace_stage_host: NULL arguments");
    return stage_run(*args);
}
