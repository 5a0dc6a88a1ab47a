// Complex products on the f64 matrix cores: the one place that spells v_mfma_f64_16x16x4_f64.
//
// One instruction is a real 16 x 16 x 4 step D = A B + C of the whole wave (verified
// on MI355X with asymmetric data, tools/probe_fp64.hip):
//   operands: lane l supplies A[row l & 15][k l >> 4] and B[k l >> 4][col l & 15], one double each;
//   result:   lane l, register r of the d4v holds D[row (l >> 4) + 4 r][col l & 15].
// A complex product is either four such steps per k-step (cmma: real and imaginary tiles) or three
// (mma3m: Gauss' P1 = Ar Br, P2 = Ai Bi, P3 = (Ar + Ai)(Br + Bi), combined once at the end by
// comb3m).  Each accumulator's chain of MFMAs is in k order, so kernels that share a helper round alike.
#pragma once

#include "ace_common.hpp"

namespace ace {

__device__ __forceinline__ d4v mfma64(double a, double b, d4v c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// (cr, ci) += a b, one complex k-step in four real products (a conjugated operand is passed conjugated:
// the negation is exact)
__device__ __forceinline__ void cmma(d4v& cr, d4v& ci, d2 a, d2 b) {
    cr = mfma64(a.x, b.x, cr);
    cr = mfma64(-a.y, b.y, cr);
    ci = mfma64(a.x, b.y, ci);
    ci = mfma64(a.y, b.x, ci);
}

// (p1, p2, p3) += a (x) b, one complex k-step of the 3M form; as = ar + ai and bs = br + bi are formed
// by the caller when an operand serves several products
__device__ __forceinline__ void mma3m(d4v& p1, d4v& p2, d4v& p3, double ar, double ai, double as, double br,
                                      double bi, double bs) {
    p1 = mfma64(ar, br, p1);
    p2 = mfma64(ai, bi, p2);
    p3 = mfma64(as, bs, p3);
}
__device__ __forceinline__ void mma3m(d4v& p1, d4v& p2, d4v& p3, d2 a, d2 b) {
    mma3m(p1, p2, p3, a.x, a.y, a.x + a.y, b.x, b.y, b.x + b.y);
}
// one element of the 3M result: (P1 - P2, P3 - P1 - P2)
__device__ __forceinline__ d2 comb3m(double e1, double e2, double e3) { return make_double2(e1 - e2, e3 - e1 - e2); }

// P[c] (3M accumulators, zeroed here) of the lane's TPW 16 x 16 output tiles of  out_i = sum_k L[i][k] v_k
// for the 16 operand rows v held in LDS (Ts, row stride tst; they are the A operand, so a result's
// row is the operand row and its column the output i).  L is in fragment order (launch_gyk_gfrag:
// [k-step][tile][lane], nct tiles, nks k-steps) and gp[c] points at the lane's entry of tile c's
// k-step 0.  SK k-steps make a stage; two register sets ping-pong, the loads of a stage issued one
// stage ahead of its MFMAs (nks / SK is even).
template <int TPW, int SK>
__device__ __forceinline__ void frag_mv(const d2* const (&gp)[TPW], const d2* Ts, int tst, int nct, int nks, int lane,
                                        d4v (&p1)[TPW], d4v (&p2)[TPW], d4v (&p3)[TPW]) {
    struct LSet {
        d2 f[SK][TPW];
    };
    struct TSet {
        d2 v[SK];
    };
    const int nstage = nks / SK;
    const d2* trow = Ts + (lane & 15) * tst + (lane >> 4);
    auto lload = [&](LSet& ls, int s) {
#pragma unroll
        for (int kk = 0; kk < SK; ++kk) {
            const long long ks = min(SK * s + kk, nks - 1);
#pragma unroll
            for (int c = 0; c < TPW; ++c) ls.f[kk][c] = gp[c][ks * nct * 64];
        }
    };
    auto tload = [&](TSet& ts, int s) {
        const int s2 = min(s, nstage - 1);
#pragma unroll
        for (int kk = 0; kk < SK; ++kk) ts.v[kk] = trow[4 * (SK * s2 + kk)];
    };
    auto comp = [&](const LSet& ls, const TSet& ts) {
#pragma unroll
        for (int kk = 0; kk < SK; ++kk) {
            const d2 v = ts.v[kk];
            const double as = v.x + v.y;
#pragma unroll
            for (int c = 0; c < TPW; ++c) {
                const d2 l = ls.f[kk][c];
                mma3m(p1[c], p2[c], p3[c], v.x, v.y, as, l.x, l.y, l.x + l.y);
            }
        }
    };
#pragma unroll
    for (int c = 0; c < TPW; ++c) p1[c] = p2[c] = p3[c] = d4v{0.0, 0.0, 0.0, 0.0};
    LSet lA, lB;
    TSet tA, tB;
    lload(lA, 0);
    tload(tA, 0);
    for (int s = 0; s < nstage; s += 2) {
        lload(lB, s + 1);
        tload(tB, s + 1);
        __builtin_amdgcn_sched_barrier(0);
        comp(lA, tA);
        __builtin_amdgcn_sched_barrier(0);
        lload(lA, s + 2);
        tload(tA, s + 2);
        __builtin_amdgcn_sched_barrier(0);
        comp(lB, tB);
        __builtin_amdgcn_sched_barrier(0);
    }
}

}  // namespace ace
