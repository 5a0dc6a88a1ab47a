// Batched min-L2 ADMM against one shared A [m][n]: InferADMM of ADMM_v2/inferMinL2.m:229-326 with lambda = 0 (the only
// value a caller passes), i.e. the 2ACE iteration with the low-rank Z-block taken out:
//   X = pinv(A) (Y - M / mu),  AX = A X,  Y = ArgMinY(AX, B, M, mu),  AtY = A^H Y,  M += mu (AX - Y),
// the best-objective iterate, the three residuals of :304-310 (sqrt(m r), sqrt(n r), sqrt(2 m r): no Z terms), the
// stop test and mu *= rho while the combined residual makes too little progress.
//
// One kernel, one launch: the initialisation and every iteration of one InferADMM call, for the whole batch.  A
// work-group (8 waves) owns 32 column slots, the columns of two MFMA tiles.  With r > 1 the slots are the <= 32 columns
// of ONE realisation (the row-mode norm, the residuals and mu couple them); with r = 1 they are the single columns of
// 32 realisations, each with its own B and its own control state.  A realisation that has stopped idles with its state
// frozen (its columns of the products are still computed and dropped); the group leaves when all of its realisations
// have stopped, at maxiter at the latest.  No host polling, no atomics, nothing is combined across work-groups.
//
// The three products of an iteration run on v_mfma_f64_16x16x4_f64 in the 4M form (cmma of ace_mfma.hpp; the values
// feed the iterate).  The matrix (pinv(A), A, or A^H read through A) is the A operand, the 32 slots of the state vector
// the B operand, the whole sum over k stays inside one wave and one accumulator chain (k ascending), and a wave
// takes the 16-row tiles w, w + 8, ...: nothing is reduced across waves.  m <= n: A pinv(A) = I, so AX = Y - M / mu
// exactly and the product is skipped.
//
// The state (S, Y, M, AX, Y_opt: m x 32; X, X_opt and two A^H Y: n x 32; complex) lives in the caller's workspace,
// [index][32 slots] per work-group.  Element phases: thread t serves slot t & 31 and the rows (t >> 5) + 16 i.  Sums
// have a fixed order: per thread in row order, the 16 partials of a slot in thread order, the slots of a realisation
// by a butterfly over the 32 lanes of their half-wave (commutative at every level, so all lanes hold the same bits;
// slots beyond the realisation's columns contribute exact zeros).  Control state (mu, last_res, opt_obj, objcol, the
// iteration count, done) is replicated per thread from those sums.  A realisation's outputs are a function of its own
// inputs, A, the sizes and the cfg alone: its columns of an MFMA result do not depend on the others, and neither the
// tile walks nor the reductions depend on its place in the batch.
//
// Setup per A (ml_setup): p = min(m, n), G = A^H A (m > n) or A A^H, R = chol(G) (launch_chol), the pivot test, and
// pinv(A) = G^-1 A^H (m > n) or A^H G^-1 by one forward and one back substitution per column.  A pivot at rounding
// level of its diagonal entry (R_jj^2 <= 64 p u G_jj) is reported as rank deficiency (ACE_ERR_UNSUPPORTED): MATLAB's
// pinv would truncate the singular value instead.
//
// The whole recovery (ml_solve: inferMinL2.m:1-227) is host code around that kernel and the pipeline's stage kernels
// (ace_pipe.hpp): normalisation and the one train partition of the batch, the spectral initialisation, the column
// count per realisation (ml_rrule_kernel), then per group of equal count the row stage, gram_rotate and the per-column
// stage, the quality on the test rows, the r = 1 refinement of the realisations above 0.6 on the full A, and finish
// (rollback, rescale).  Grouping does not change a realisation's outputs, by the property above.
//
// No dynamic LDS (ace_lds_request "minl2" is 0 at every m); 16 KiB static in the loop kernel (the reductions); no
// scratch (profiles/minl2_resources.json).
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"
#include "ace_phaselift.hpp"
#include "ace_pipe.hpp"

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

namespace ace {
namespace {

constexpr int ML_WAVES = 8;
constexpr int ML_NT = 64 * ML_WAVES;
constexpr int ML_CS = 32;                // column slots of a work-group
constexpr int ML_TR = ML_NT / ML_CS;     // threads of a slot
constexpr int ML_NMAX = 1024;
constexpr int ML_MMAX = 4096;
constexpr int ML_RMAX = 32;
constexpr int ML_RK = 4;                 // sums per reduction
static_assert(ML_TR == 16 && ML_RMAX == ML_CS, "thread layout");

struct MinL2Args {
    int batch, m, n, r, spr, row_mode, maxiter;   // spr: slots per realisation, 32 (r > 1) or 1
    double mu0, rho, tol_rel, tol_abs;
    const d2* A;
    const d2* U;   // pinv(A) [n][m]
    const double* B;
    const d2* X0;
    const int32_t* rcols;
    d2* X;
    d2* Y;
    d2* Xall;
    int32_t* iters;
    int32_t* objcol;
    double* opt_obj;
    double* mu;
    uint32_t* status;
    d2* ws;
};

// complex elements of a work-group's state
constexpr size_t ml_group_elems(int m, int n) { return ((size_t)5 * m + (size_t)4 * n) * ML_CS; }

// out[i][s] = sum_k L(i, k) V[k][s] for i < rows, k < K and the 32 slots s.  TR = false: L(i, k) = Lp[i K + k];
// TR = true: L = Lp^H with Lp [K][rows].  Wave w takes the row tiles w, w + 8, ...; lane l supplies L(16 rt + (l & 15),
// k0 + (l >> 4)) and V[k0 + (l >> 4)][(l & 15), 16 + (l & 15)] and receives rows 16 rt + (l >> 4) + 4 q.
template <bool TR>
__device__ __forceinline__ void ml_prod(const d2* __restrict__ Lp, int rows, int K, const d2* V, d2* out, int w, int lane) {
    const int li = lane & 15, lk = lane >> 4;
    const int ntile = (rows + 15) / 16;
    for (int rt = w; rt < ntile; rt += ML_WAVES) {
        const int i = min(16 * rt + li, rows - 1);   // (a tile's rows beyond the matrix repeat its last one and are dropped)
        d4v cr0 = d4v{0.0, 0.0, 0.0, 0.0}, ci0 = cr0, cr1 = cr0, ci1 = cr0;
        auto lload = [&](int k) {
            if (TR) {
                const d2 c = Lp[(size_t)k * rows + i];
                return make_double2(c.x, -c.y);
            }
            return Lp[(size_t)i * K + k];
        };
        const int Kf = K & ~3;
        for (int k0 = 0; k0 < Kf; k0 += 4) {
            const int k = k0 + lk;
            const d2 l = lload(k);
            cmma(cr0, ci0, l, V[(size_t)k * ML_CS + li]);
            cmma(cr1, ci1, l, V[(size_t)k * ML_CS + 16 + li]);
        }
        if (Kf < K) {   // the last, partial k-step: zeros beyond K on both sides
            const int k = Kf + lk;
            d2 l = make_double2(0.0, 0.0), v0 = l, v1 = l;
            if (k < K) {
                l = lload(k);
                v0 = V[(size_t)k * ML_CS + li];
                v1 = V[(size_t)k * ML_CS + 16 + li];
            }
            cmma(cr0, ci0, l, v0);
            cmma(cr1, ci1, l, v1);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = 16 * rt + lk + 4 * q;
            if (row < rows) {
                out[(size_t)row * ML_CS + li] = make_double2(cr0[q], ci0[q]);
                out[(size_t)row * ML_CS + 16 + li] = make_double2(cr1[q], ci1[q]);
            }
        }
    }
}

// v[k] <- the sum over the 16 threads of the slot, in thread order: the same bits in all of them
template <int K>
__device__ __forceinline__ void ml_red(double (&v)[K], double* red, int t) {
    static_assert(K <= ML_RK, "reduction buffer");
#pragma unroll
    for (int k = 0; k < K; ++k) red[(k * ML_TR + (t >> 5)) * ML_CS + (t & 31)] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < ML_TR; ++i) s += red[(k * ML_TR + i) * ML_CS + (t & 31)];
        v[k] = s;
    }
    __syncthreads();
}

// p[i] where ok, else 0 (as a value: a conditional between two d2 objects selects between their addresses and puts the
// constant into scratch)
__device__ __forceinline__ d2 ml_ld(bool ok, const d2* p, size_t i) {
    d2 v = make_double2(0.0, 0.0);
    if (ok) v = p[i];
    return v;
}

// the sum over the 32 slots of the lane's half-wave (every lane takes part and gets the same bits)
__device__ __forceinline__ double ml_xs(double v) {
#pragma unroll
    for (int o = 1; o < ML_CS; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(ML_NT) void minl2_kernel(const MinL2Args a) {
    __shared__ double red[ML_RK * ML_TR * ML_CS];
    const int m = a.m, n = a.n;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int s = t & 31, tr = t >> 5;
    const bool wide = a.spr == ML_CS;                  // one realisation per group
    const long long b = wide ? (long long)blockIdx.x : (long long)blockIdx.x * ML_CS + s;
    const int c = wide ? s : 0;                        // the slot's column of its realisation
    const bool live = b < a.batch;
    int rc = 0;
    if (live) {
        rc = a.r;
        if (a.rcols) rc = min(max(a.rcols[b], 1), a.r);
    }
    const bool col_on = live && c < rc;
    const bool row_mode = a.row_mode != 0;

    d2* const S = a.ws + (size_t)blockIdx.x * ml_group_elems(m, n);
    d2* const Y = S + (size_t)m * ML_CS;
    d2* const M = Y + (size_t)m * ML_CS;
    d2* const AXb = M + (size_t)m * ML_CS;
    d2* const YO = AXb + (size_t)m * ML_CS;
    d2* const XW = YO + (size_t)m * ML_CS;
    d2* const XO = XW + (size_t)n * ML_CS;
    d2* const G0 = XO + (size_t)n * ML_CS;
    d2* const G1 = G0 + (size_t)n * ML_CS;
    const d2* const AXp = m > n ? AXb : S;             // m <= n: A pinv(A) = I
    const double* const Bb = a.B + (live ? (size_t)b * m : 0);

    // ---------------- init (:244-257): X0 scaled to ||A X|| = ||B||, Y = normalize_rows(A X, B), A^H Y, M = 0
    for (int j = tr; j < n; j += ML_TR) XW[(size_t)j * ML_CS + s] = ml_ld(col_on, a.X0, ((size_t)b * a.r + c) * n + j);
    __syncthreads();
    ml_prod<false>(a.A, m, n, XW, AXb, w, lane);
    __syncthreads();
    {
        double v[2] = {0.0, 0.0};
        for (int e = tr; e < m; e += ML_TR) {
            v[0] += cabs2(AXb[(size_t)e * ML_CS + s]);
            const double bv = live ? Bb[e] : 0.0;
            v[1] += bv * bv;
        }
        ml_red(v, red, t);
        double nax2 = col_on ? v[0] : 0.0;
        if (wide && row_mode) nax2 = ml_xs(nax2);
        const double sc = sqrt(v[1]) / sqrt(nax2);
        for (int j = tr; j < n; j += ML_TR)
            if (col_on) XW[(size_t)j * ML_CS + s] = cscale(XW[(size_t)j * ML_CS + s], sc);
    }
    __syncthreads();
    ml_prod<false>(a.A, m, n, XW, AXb, w, lane);
    __syncthreads();
    for (int e0 = 0; e0 < m; e0 += ML_TR) {
        const int e = e0 + tr;
        const bool in = e < m;
        const size_t i = (size_t)(in ? e : 0) * ML_CS + s;
        d2 y = ml_ld(in && col_on, AXb, i);
        const double bv = in && live ? Bb[e] : 0.0;
        double D;
        if (row_mode) {
            double q = cabs2(y);
            if (wide) q = ml_xs(q);
            D = sqrt(q);
            if (D == 0.0) {
                y = make_double2(1.0 / sqrt((double)rc), 0.0);
                D = 1.0;
            }
        } else {
            D = sqrt(cabs2(y));
            if (D == 0.0) {
                y = make_double2(1.0, 0.0);
                D = 1.0;
            }
        }
        if (in) {
            const double f = col_on ? bv / D : 0.0;
            Y[i] = make_double2(col_on ? y.x * f : 0.0, col_on ? y.y * f : 0.0);
            M[i] = make_double2(0.0, 0.0);
            S[i] = make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    ml_prod<true>(a.A, n, m, Y, G0, w, lane);
    __syncthreads();

    // ---------------- the iterations (:266-322)
    double mu = a.mu0, last_res = INFINITY, opt_obj = INFINITY;
    int it = 0, objcol = 0, cur = 0;
    bool done = !live, conv = false, have_opt = false;
    while (true) {
        if (__syncthreads_or(!done) == 0) break;
        const bool act = !done && col_on;
        if (!done) ++it;
        d2* const Gold = cur ? G1 : G0;
        d2* const Gnew = cur ? G0 : G1;
        // X = pinv(A) (Y - M / mu), AX = A X
        for (int e = tr; e < m; e += ML_TR) {
            const size_t i = (size_t)e * ML_CS + s;
            if (act) {
                const d2 mm = M[i];
                S[i] = csub(Y[i], make_double2(mm.x / mu, mm.y / mu));
            }
        }
        __syncthreads();
        ml_prod<false>(a.U, n, m, S, XW, w, lane);
        __syncthreads();
        if (m > n) {
            ml_prod<false>(a.A, m, n, XW, AXb, w, lane);
            __syncthreads();
        }
        // Y = ArgMinY (:371-393), M += mu (AX - Y), the sums of the residuals and of the objective
        double v[4] = {0.0, 0.0, 0.0, 0.0}, o[1] = {0.0};
        for (int e0 = 0; e0 < m; e0 += ML_TR) {
            const int e = e0 + tr;
            const bool in = e < m;
            const size_t i = (size_t)(in ? e : 0) * ML_CS + s;
            const bool on = in && col_on;
            const d2 ax = ml_ld(on, AXp, i);
            const d2 mm = ml_ld(on, M, i);
            const d2 yold = ml_ld(on, Y, i);
            const double bv = in && live ? Bb[e] : 0.0;
            d2 cc = cadd(ax, make_double2(mm.x / mu, mm.y / mu));
            const double ax2 = cabs2(ax);
            double D, dobj;
            if (row_mode) {
                double q = cabs2(cc), q2 = ax2;
                if (wide) {
                    q = ml_xs(q);
                    q2 = ml_xs(q2);
                }
                D = sqrt(q);
                if (D == 0.0) {
                    cc = make_double2(1.0 / sqrt((double)rc), 0.0);
                    D = 1.0;
                }
                dobj = c == 0 ? sqrt(q2) - bv : 0.0;
            } else {
                D = sqrt(cabs2(cc));
                if (D == 0.0) {
                    cc = make_double2(1.0, 0.0);
                    D = 1.0;
                }
                dobj = sqrt(ax2) - bv;
            }
            const d2 yn = cscale(cc, (bv / D + mu) / (1.0 + mu));
            const d2 J = csub(ax, yn);
            if (on) {
                v[0] += cabs2(J);
                v[1] += cabs2(csub(yn, yold));
                v[2] += ax2;
                v[3] += cabs2(yn);
                o[0] += dobj * dobj;
                if (act) {
                    Y[i] = yn;
                    M[i] = cadd(mm, cscale(J, mu));
                }
            }
        }
        ml_red(v, red, t);
        ml_red(o, red, t);   // (its barriers also order the stores of Y before the product's loads)
        ml_prod<true>(a.A, n, m, Y, Gnew, w, lane);
        __syncthreads();
        double g[2] = {0.0, 0.0};
        for (int j = tr; j < n; j += ML_TR) {
            const size_t i = (size_t)j * ML_CS + s;
            if (col_on) {
                const d2 gn = Gnew[i];
                g[0] += cabs2(csub(gn, Gold[i]));
                g[1] += cabs2(gn);
            }
        }
        ml_red(g, red, t);
        if (wide) {   // Frobenius norms over the realisation's columns
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = ml_xs(col_on ? v[k] : 0.0);
            g[0] = ml_xs(col_on ? g[0] : 0.0);
            g[1] = ml_xs(col_on ? g[1] : 0.0);
        }
        // the objective (:284-301): the row form, or the first smallest column, NaN skipped as MATLAB's min does
        double obj;
        int oj = 0;
        if (row_mode) {
            obj = sqrt(wide ? ml_xs(col_on ? o[0] : 0.0) : o[0]);
        } else if (wide) {
            const double mine = sqrt(o[0]);
            obj = NAN;
            for (int k = 0; k < rc; ++k) {
                const double ok = __shfl(mine, (lane & 32) | k, 64);
                if (!isnan(ok) && (isnan(obj) || ok < obj)) {
                    obj = ok;
                    oj = k;
                }
            }
        } else {
            obj = sqrt(o[0]);
        }
        if (!done && obj < opt_obj) {
            opt_obj = obj;
            objcol = oj;
            have_opt = true;
            if (col_on) {
                for (int j = tr; j < n; j += ML_TR) XO[(size_t)j * ML_CS + s] = XW[(size_t)j * ML_CS + s];
                for (int e = tr; e < m; e += ML_TR) YO[(size_t)e * ML_CS + s] = Y[(size_t)e * ML_CS + s];
            }
        }
        // the stop test (:304-315) and the mu update (:318-321)
        if (!done) {
            const double res_prim = sqrt(v[0]), res_dual = mu * sqrt(g[0]), ny0 = sqrt(v[1]);
            const double res_comb = sqrt(res_prim * res_prim + ny0 * ny0);
            const double nax = sqrt(v[2]), ny = sqrt(v[3]), naty = sqrt(g[1]);
            const double mx = fmax(nax, ny);
            const double mr = (double)m * rc, nr = (double)n * rc;
            const double th_prim = a.tol_abs * sqrt(mr) + a.tol_rel * mx;
            const double th_dual = a.tol_abs * sqrt(nr) + a.tol_rel * naty;
            const double th_comb = a.tol_abs * sqrt(mr * 2.0) + a.tol_rel * sqrt(mx * mx + ny * ny);
            if ((res_prim < th_prim && res_dual < th_dual) || res_comb < th_comb) {
                conv = true;
                done = true;
            } else {
                if (res_comb > last_res * 0.9) mu *= a.rho;
                last_res = res_comb;
                if (it >= a.maxiter) done = true;
            }
        }
        cur ^= 1;
    }

    // ---------------- outputs: the best iterate (the last one where the objective was never finite)
    if (!live) return;
    const d2* const Xs = have_opt ? XO : XW;
    const d2* const Ys = have_opt ? YO : Y;
    if (wide ? c < a.r : true) {
        if (row_mode) {
            for (int j = tr; j < n; j += ML_TR) a.X[((size_t)b * a.r + c) * n + j] = ml_ld(col_on, Xs, (size_t)j * ML_CS + s);
            if (a.Y)   // (absent for the row stage of the whole recovery)
                for (int e = tr; e < m; e += ML_TR) a.Y[((size_t)b * a.r + c) * m + e] = ml_ld(col_on, Ys, (size_t)e * ML_CS + s);
        } else if (c == objcol) {
            for (int j = tr; j < n; j += ML_TR) a.X[(size_t)b * n + j] = Xs[(size_t)j * ML_CS + s];
            for (int e = tr; e < m; e += ML_TR) a.Y[(size_t)b * m + e] = Ys[(size_t)e * ML_CS + s];
        }
        if (a.Xall)
            for (int j = tr; j < n; j += ML_TR) a.Xall[((size_t)b * a.r + c) * n + j] = ml_ld(col_on, Xs, (size_t)j * ML_CS + s);
    }
    if (tr == 0 && c == 0) {
        if (a.iters) a.iters[b] = it;
        if (a.objcol) a.objcol[b] = objcol;
        if (a.opt_obj) a.opt_obj[b] = opt_obj;
        if (a.mu) a.mu[b] = mu;
        if (a.status) a.status[b] = (conv ? ACE_ST_CONVERGED : 0u) | (have_opt ? 0u : ACE_ST_NO_OPT);
    }
}

// ---------------- setup per A
// G = A^H A (m > n) or A A^H, p x p with p = min(m, n); the upper triangle is what launch_chol reads
__global__ __launch_bounds__(256) void ml_gram_kernel(int m, int n, const d2* __restrict__ A, d2* G) {
    const int p = m > n ? n : m;
    const int i = blockIdx.y * 16 + (threadIdx.x >> 4), j = blockIdx.x * 16 + (threadIdx.x & 15);
    if (i >= p || j >= p) return;
    d2 acc = make_double2(0.0, 0.0);
    if (m > n)
        for (int e = 0; e < m; ++e) acc = cadd(acc, cmulc(A[(size_t)e * n + i], A[(size_t)e * n + j]));
    else
        for (int k = 0; k < n; ++k) acc = cadd(acc, cmulc(A[(size_t)j * n + k], A[(size_t)i * n + k]));
    G[(size_t)i * p + j] = acc;
}

// ok[0] <- 0 where a pivot of R = chol(G) is at rounding level of its diagonal entry
__global__ __launch_bounds__(256) void ml_pivot_kernel(int p, const d2* G, const d2* R, int* ok) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const double lim = 64.0 * p * 0x1p-53;
    for (int j = threadIdx.x; j < p; j += 256) {
        const double rjj = R[(size_t)j * p + j].x, gjj = G[(size_t)j * p + j].x;
        if (!(rjj * rjj > lim * gjj)) bad = 1;   // (a benign race: every writer stores 1)
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad) ok[0] = 0;
}

// column q of pinv(A) through G = R^H R: G^-1 conj(A[q][:]) (m > n, q < m) or conj(G^-1 A[:][q]) (q < n)
__global__ __launch_bounds__(256) void ml_pinv_kernel(int m, int n, const d2* __restrict__ A, const d2* __restrict__ R, d2* U) {
    __shared__ d2 wv[ML_NMAX];
    __shared__ d2 wj;
    const bool tall = m > n;
    const int p = tall ? n : m, q = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < p; i += 256) {
        const d2 v = tall ? A[(size_t)q * n + i] : A[(size_t)i * n + q];
        wv[i] = tall ? make_double2(v.x, -v.y) : v;
    }
    __syncthreads();
    for (int j = 0; j < p; ++j) {   // R^H z = w, column-oriented
        if (t == 0) {
            wj = cscale(wv[j], 1.0 / R[(size_t)j * p + j].x);
            wv[j] = wj;
        }
        __syncthreads();
        const d2 cj = wj;
        for (int i = j + 1 + t; i < p; i += 256) wv[i] = csub(wv[i], cmulc(R[(size_t)j * p + i], cj));
        __syncthreads();
    }
    for (int j = p - 1; j >= 0; --j) {   // R u = z
        if (t == 0) {
            wj = cscale(wv[j], 1.0 / R[(size_t)j * p + j].x);
            wv[j] = wj;
        }
        __syncthreads();
        const d2 cj = wj;
        for (int i = t; i < j; i += 256) wv[i] = csub(wv[i], cmul(R[(size_t)i * p + j], cj));
        __syncthreads();
    }
    for (int i = t; i < p; i += 256) {
        const d2 v = wv[i];
        if (tall) U[(size_t)i * m + q] = v;
        else U[(size_t)q * m + i] = make_double2(v.x, -v.y);
    }
}

struct MlSetup {
    d2 *U, *G, *R;
    int* ok;
};
void ml_carve_setup(Carver& cv, int m, int n, MlSetup* su) {
    const size_t p = m > n ? n : m;
    su->U = cv.take<d2>(sizeof(d2) * (size_t)n * m);
    su->G = cv.take<d2>(sizeof(d2) * p * p);
    su->R = cv.take<d2>(sizeof(d2) * p * p);
    su->ok = cv.take<int>(256);
}
size_t ml_groups(int batch, int r) { return r > 1 ? (size_t)batch : ((size_t)batch + ML_CS - 1) / ML_CS; }
size_t ml_ws_bytes(int batch, int m, int n, int r) {
    Carver cv{nullptr};
    MlSetup su;
    ml_carve_setup(cv, m, n, &su);
    cv.take<d2>(sizeof(d2) * ml_groups(batch, r) * ml_group_elems(m, n));
    return cv.off + 256;   // (the base is aligned up)
}

// pinv(A) into su.U; ACE_ERR_UNSUPPORTED for a rank-deficient A (synchronises the stream once)
int ml_setup(int m, int n, const double* A, const MlSetup& su, hipStream_t st) {
    const int p = m > n ? n : m;
    hipLaunchKernelGGL(ml_gram_kernel, dim3((p + 15) / 16, (p + 15) / 16), dim3(256), 0, st, m, n, (const d2*)A, su.G);
    launch_chol(p, (const double*)su.G, (double*)su.R, su.ok, st);
    hipLaunchKernelGGL(ml_pivot_kernel, dim3(1), dim3(256), 0, st, p, su.G, su.R, su.ok);
    ACE_HIP(hipGetLastError());
    int ok = 0;
    ACE_HIP(read_back(&ok, su.ok, sizeof(int), st));
    if (!ok)
        return fail(ACE_ERR_UNSUPPORTED, "minl2: A (%d x %d) is rank deficient (chol(%s) met a pivot at rounding level); "
                    "pinv would truncate it", m, n, m > n ? "A^H A" : "A A^H");
    hipLaunchKernelGGL(ml_pinv_kernel, dim3(m > n ? m : n), dim3(256), 0, st, m, n, (const d2*)A, su.R, su.U);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

int ml_check_cfg(const ace_minl2_cfg* cfg) {
    if (!cfg) return fail(ACE_ERR_ARG, "minl2: NULL cfg");
    if (cfg->maxiter < 1) return fail(ACE_ERR_ARG, "minl2: maxiter %d < 1", cfg->maxiter);
    if (!(cfg->mu0 > 0.0) || !(cfg->rho > 0.0)) return fail(ACE_ERR_ARG, "minl2: mu0 %g and rho %g must be positive", cfg->mu0, cfg->rho);
    if (!(cfg->tol_rel >= 0.0) || !(cfg->tol_abs >= 0.0)) return fail(ACE_ERR_ARG, "minl2: negative tolerance");
    return ACE_OK;
}
int ml_check_sizes(int batch, int m, int n, int r) {
    if (batch < 1) return fail(ACE_ERR_ARG, "minl2: batch %d < 1", batch);
    if (m < 1 || m > ML_MMAX) return fail(ACE_ERR_ARG, "minl2: m %d outside 1..%d", m, ML_MMAX);
    if (n < 1 || n > ML_NMAX) return fail(ACE_ERR_ARG, "minl2: n %d outside 1..%d", n, ML_NMAX);
    if (r < 1 || r > ML_RMAX) return fail(ACE_ERR_ARG, "minl2: r %d outside 1..%d", r, ML_RMAX);
    return ACE_OK;
}
int ml_check_stage(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int scale_by_row, const double* A,
                   const double* B, const double* X0, const double* X, const double* Y) {
    ACE_TRY(ml_check_cfg(cfg));
    ACE_TRY(ml_check_sizes(batch, m, n, r));
    if (scale_by_row != 0 && scale_by_row != 1) return fail(ACE_ERR_ARG, "minl2: scale_by_row %d is not 0 or 1", scale_by_row);
    if (!A || !B || !X0 || !X || !Y) return fail(ACE_ERR_ARG, "minl2: NULL %s", !A ? "A" : !B ? "B" : !X0 ? "X0" : !X ? "X" : "Y");
    return ACE_OK;
}

void ml_launch(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int row_mode, const double* A, const d2* U,
               const double* B, const double* X0, const int32_t* rcols, double* X, double* Y, double* Xall, int32_t* iters,
               int32_t* objcol, double* opt_obj, double* mu, uint32_t* status, d2* ws, hipStream_t st) {
    MinL2Args a;
    a.batch = batch;
    a.m = m;
    a.n = n;
    a.r = r;
    a.spr = r > 1 ? ML_CS : 1;
    a.row_mode = row_mode;
    a.maxiter = cfg->maxiter;
    a.mu0 = cfg->mu0;
    a.rho = cfg->rho;
    a.tol_rel = cfg->tol_rel;
    a.tol_abs = cfg->tol_abs;
    a.A = (const d2*)A;
    a.U = U;
    a.B = B;
    a.X0 = (const d2*)X0;
    a.rcols = rcols;
    a.X = (d2*)X;
    a.Y = (d2*)Y;
    a.Xall = (d2*)Xall;
    a.iters = iters;
    a.objcol = objcol;
    a.opt_obj = opt_obj;
    a.mu = mu;
    a.status = status;
    a.ws = ws;
    hipLaunchKernelGGL(minl2_kernel, dim3((unsigned)ml_groups(batch, r)), dim3(ML_NT), 0, st, a);
}


// ---------------- the whole recovery (inferMinL2.m:1-227)
// dst[k][0 .. len) = src[idx[k]][0 .. len) with rows of sstride (source) and len (destination) doubles
__global__ __launch_bounds__(256) void ml_gather_kernel(long long len, const double* src, long long sstride, double* dst,
                                                        const int* idx) {
    const long long so = (long long)idx[blockIdx.x] * sstride, dof = (long long)blockIdx.x * len;
    for (long long e = threadIdx.x; e < len; e += 256) dst[dof + e] = src[so + e];
}

// Y3[b] = (Y2[b] on the m_t train rows, 0 beyond): the Y of a recovery without refinement
__global__ __launch_bounds__(256) void ml_pad_y_kernel(int m, int mt, const d2* Y2, d2* Y3) {
    const long long b = blockIdx.x;
    for (int i = threadIdx.x; i < m; i += 256) Y3[b * m + i] = i < mt ? Y2[b * mt + i] : make_double2(0.0, 0.0);
}

// The column count of :187-190 per realisation from the spectral initialisation's columns X0 [batch][rs][n]
// (column k = sqrt(s2_k) v_k, descending): s2_k = ||column k||^2 and sum(s2) = trace(As^H As) = the sum of B_i^2 over
// the rows of A_t that are not zero.  rs = min(max(r, 3), m_t, n) columns are computed: beyond m_t the spectrum is zero,
// and the rule's floor of 3 can ask for more columns than r < 3 (the reference takes a third eigenvector there).  The
// copy of the block at :203-206 changes nothing: where the first block fired, the second either does not fire and keeps
// the count, or fires and computes the same one from the same cumulative sum.
__global__ __launch_bounds__(256) void ml_rrule_kernel(int mt, int n, int r0, int rs, const d2* At, const double* Bt,
                                                       const d2* X0, int* rc) {
    __shared__ double sh[16 * 2];
    __shared__ double s2[ML_RMAX];
    const int b = blockIdx.x, t = threadIdx.x;
    double v[1] = {0.0};
    for (int i = t; i < mt; i += 256) {
        bool nz = false;
        for (int j = 0; j < n && !nz; ++j) nz = cabs2(At[(size_t)i * n + j]) != 0.0;
        const double bi = Bt[(size_t)b * mt + i];
        if (nz) v[0] += bi * bi;
    }
    block_sum<1>(v, sh);
    const double tot = v[0];
    for (int k = 0; k < rs; ++k) {
        double q[1] = {0.0};
        for (int j = t; j < n; j += 256) q[0] += cabs2(X0[((size_t)b * rs + k) * n + j]);
        block_sum<1>(q, sh);
        if (t == 0) s2[k] = q[0];
    }
    __syncthreads();
    if (t == 0) {
        const int rt = min(r0, rs);   // sum(s2(1:r)): the entries beyond m_t are zero
        double top = 0.0;
        for (int k = 0; k < rt; ++k) top += s2[k];
        int r = rt;
        if (top >= tot * 0.9) {
            double cum = 0.0;
            int k90 = rs;
            for (int k = 0; k < rs; ++k) {
                cum += s2[k];
                if (cum >= tot * 0.9) {
                    k90 = k + 1;
                    break;
                }
            }
            r = max(k90, 3);
            r = min(r, min(mt, n));
        }
        rc[b] = r;
    }
}

struct MlDims {
    int batch, m, n, r, mt, mte, rs;
};
int ml_dims(const ace_minl2_cfg* cfg, int batch, int m, int n, MlDims* d) {
    ACE_TRY(ml_check_cfg(cfg));
    if (cfg->r < 1) return fail(ACE_ERR_ARG, "minl2: r %d < 1", cfg->r);
    if (!(cfg->cc_frac > 0.0 && cfg->cc_frac <= 1.0)) return fail(ACE_ERR_ARG, "minl2: cc_frac %g outside (0, 1]", cfg->cc_frac);
    const int r = std::min(cfg->r, std::min(m, n));
    ACE_TRY(ml_check_sizes(batch, m, n, r < 1 ? 1 : r));
    d->batch = batch;
    d->m = m;
    d->n = n;
    d->r = r;
    d->mt = std::max(1, std::min(m, (int)std::ceil(m * cfg->cc_frac)));
    d->mte = m - d->mt;
    d->rs = std::min(std::max(r, 3), std::min(d->mt, n));   // the columns of the spectral initialisation (ml_rrule_kernel)
    return ACE_OK;
}

struct MlSolveWs {
    MlSetup su;
    double *anorm, *bnorm, *Bn, *At, *Ate, *An, *Bt, *Bte, *AH, *K, *spec, *W, *X0, *q;
    int *rows, *rc, *gidx, *gall, *ist, *iit, *st2;
    double *Bg, *X0g, *X1g, *Xg, *Yg, *X2, *Y2, *X3, *Y3;
    d2* state;
};
void ml_carve_solve(Carver& cv, const MlDims& d, MlSolveWs* w) {
    const size_t B = d.batch, m = d.m, n = d.n, mt = d.mt, mte = d.mte, rs = d.rs;
    ml_carve_setup(cv, d.m, d.n, &w->su);
    w->anorm = cv.take(256);
    w->bnorm = cv.take(8 * B);
    w->Bn = cv.take(8 * B * m);
    w->At = cv.take(16 * mt * n);
    w->Ate = cv.take(16 * (mte ? mte : 1) * n);
    w->An = cv.take(16 * m * n);
    w->Bt = cv.take(8 * B * mt);
    w->Bte = cv.take(8 * B * (mte ? mte : 1));
    w->AH = cv.take(16 * mt * n);
    w->K = cv.take(16 * mt * mt);
    w->spec = cv.take(spectral_scratch_bytes(d.mt, d.n, d.batch, d.rs));
    w->W = cv.take(spectral_primal(d.mt, d.n) ? 256 : 16 * B * rs * mt);
    w->X0 = cv.take(16 * B * rs * n);
    w->q = cv.take(8 * B);
    w->rows = cv.take<int>(4 * 2 * m);
    w->rc = cv.take<int>(4 * B);
    w->gidx = cv.take<int>(4 * B);
    w->gall = cv.take<int>(4 * B);
    w->ist = cv.take<int>(4 * B);
    w->iit = cv.take<int>(4 * B);
    w->st2 = cv.take<int>(4 * B);
    w->Bg = cv.take(8 * B * m);
    w->X0g = cv.take(16 * B * rs * n);
    w->X1g = cv.take(16 * B * rs * n);
    w->Xg = cv.take(16 * B * n);
    w->Yg = cv.take(16 * B * m);
    w->X2 = cv.take(16 * B * n);
    w->Y2 = cv.take(16 * B * mt);
    w->X3 = cv.take(16 * B * n);
    w->Y3 = cv.take(16 * B * m);
    const size_t g12 = ml_groups(d.batch, 2) * ml_group_elems(d.mt, d.n), g3 = ml_groups(d.batch, 1) * ml_group_elems(d.m, d.n);
    w->state = cv.take<d2>(sizeof(d2) * std::max(g12, g3));
}
size_t ml_solve_bytes(const MlDims& d) {
    Carver cv{nullptr};
    MlSolveWs w;
    ml_carve_solve(cv, d, &w);
    return cv.off + 256;
}

// rows: the m_t train rows as given, then the test rows ascending (setdiff, :35); then the identity
int ml_partition(const ace_minl2_cfg* cfg, const MlDims& d, const int32_t* train_idx, std::vector<int>* rows) {
    std::vector<int32_t> drawn;
    if (!train_idx) {
        drawn.resize(d.mt);
        (void)ace_driver_randperm((uint64_t)(uint32_t)cfg->train_seed, 0, d.m, d.mt, drawn.data());
        train_idx = drawn.data();
    }
    std::vector<char> seen(d.m, 0);
    rows->clear();
    for (int k = 0; k < d.mt; ++k) {
        const int v = train_idx[k];
        if (v < 0 || v >= d.m || seen[v]) return fail(ACE_ERR_ARG, "minl2: train_idx[%d] = %d: out of range or repeated", k, v);
        seen[v] = 1;
        rows->push_back(v);
    }
    for (int v = 0; v < d.m; ++v)
        if (!seen[v]) rows->push_back(v);
    for (int v = 0; v < d.m; ++v) rows->push_back(v);
    return ACE_OK;
}

int ml_solve(const ace_minl2_cfg* cfg, const MlDims& d, const std::vector<int>& rows, const double* A, const double* B,
             double* X, double* Y, double* quality, int32_t* stage_iters, int32_t* r_used, uint32_t* status,
             const MlSolveWs& w, hipStream_t st) {
    const int batch = d.batch, m = d.m, n = d.n, mt = d.mt, mte = d.mte, rs = d.rs;
    ACE_HIP(upload(w.rows, rows.data(), sizeof(int) * 2 * (size_t)m, st));
    ACE_HIP(hipMemsetAsync(w.ist, 0, sizeof(int) * (size_t)batch, st));
    if (stage_iters) ACE_HIP(hipMemsetAsync(stage_iters, 0, sizeof(int32_t) * 3 * (size_t)batch, st));
    // ---- :14-39: normalise, partition
    launch_anorm(m, n, A, cfg->tol_abs, w.anorm, st);
    launch_bnorm(m, batch, B, cfg->tol_abs, w.bnorm, w.Bn, st);
    launch_gather_rows(mt, n, A, w.rows, w.anorm, w.At, st);
    if (mte) launch_gather_rows(mte, n, A, w.rows + mt, w.anorm, w.Ate, st);
    launch_gather_rows(m, n, A, w.rows + m, w.anorm, w.An, st);
    launch_gather_b(m, mt, batch, w.Bn, w.rows, w.Bt, st);
    if (mte) launch_gather_b(m, mte, batch, w.Bn, w.rows + mt, w.Bte, st);
    // ---- :176-207: the spectral initialisation and the column count
    launch_conj_transpose(mt, n, w.At, w.AH, st);
    launch_zgemm(0, true, mt, n, mt, w.At, n, 0, w.At, n, 0, w.K, nullptr, mt, 0, 1, st);   // K = A_t A_t^H
    if (spectral_primal(mt, n)) {
        if (launch_spectral_primal(mt, n, rs, batch, w.K, w.AH, w.Bt, w.spec, w.X0, w.ist, st))
            return fail(ACE_ERR_UNSUPPORTED, "minl2: spectral initialisation: n = %d too large", n);
    } else {
        if (launch_spectral(mt, rs, batch, w.K, w.Bt, w.spec, w.W, w.ist, st))
            return fail(ACE_ERR_UNSUPPORTED, "minl2: spectral initialisation: m_t = %d too large", mt);
        launch_zgemm(0, false, n, mt, batch * rs, w.AH, mt, 0, w.W, mt, 0, w.X0, nullptr, n, 0, 1, st);
    }
    ACE_LAUNCHED("minl2 spectral initialisation");
    hipLaunchKernelGGL(ml_rrule_kernel, dim3(batch), dim3(256), 0, st, mt, n, d.r, rs, (const d2*)w.At, w.Bt, (const d2*)w.X0, w.rc);
    std::vector<int> rc(batch);
    ACE_HIP(read_back(rc.data(), w.rc, sizeof(int) * (size_t)batch, st));
    if (r_used) ACE_HIP(hipMemcpyAsync(r_used, w.rc, sizeof(int) * (size_t)batch, hipMemcpyDeviceToDevice, st));
    if (status) launch_put_col(batch, w.ist, nullptr, (int*)status, 1, 0, 0u, st);   // (ACE_ST_EIG_NOCONV of the init)
    // ---- :213-225 per column count: the row stage, the rotation by eig(X^H X), the per-column stage
    ACE_TRY(ml_setup(mt, n, w.At, w.su, st));
    std::map<int, std::vector<int>> groups;
    for (int b = 0; b < batch; ++b) {
        if (rc[b] < 1 || rc[b] > rs) return fail(ACE_ERR_HIP, "minl2: column count %d of realisation %d outside 1..%d", rc[b], b, rs);
        groups[rc[b]].push_back(b);
    }
    std::vector<int> order;   // the groups' members one after the other: one upload
    for (const auto& g : groups) order.insert(order.end(), g.second.begin(), g.second.end());
    ACE_HIP(upload(w.gall, order.data(), sizeof(int) * (size_t)batch, st));
    int goff = 0;
    for (const auto& g : groups) {
        const int rg = g.first, cnt = (int)g.second.size();
        const int* const gidx = w.gall + goff;
        goff += cnt;
        hipLaunchKernelGGL(ml_gather_kernel, dim3(cnt), dim3(256), 0, st, (long long)mt, w.Bt, (long long)mt, w.Bg, gidx);
        hipLaunchKernelGGL(ml_gather_kernel, dim3(cnt), dim3(256), 0, st, 2LL * rg * n, w.X0, 2LL * rs * n, w.X0g, gidx);
        ml_launch(cfg, cnt, mt, n, rg, 1, w.At, w.su.U, w.Bg, w.X0g, nullptr, w.X1g, nullptr, nullptr, w.iit, nullptr, nullptr,
                  nullptr, (uint32_t*)w.ist, w.state, st);
        if (stage_iters) launch_put_col(cnt, w.iit, gidx, stage_iters, 3, 0, 0u, st);
        if (status) launch_put_col(cnt, w.ist, gidx, (int*)status, 1, 0, ACE_ST_NO_OPT, st);
        ACE_HIP(hipMemsetAsync(w.ist, 0, sizeof(int) * (size_t)cnt, st));
        launch_gram_rotate(n, rg, cnt, w.X1g, w.ist, st);
        if (status) launch_put_col(cnt, w.ist, gidx, (int*)status, 1, 0, ACE_ST_EIG_NOCONV, st);
        ml_launch(cfg, cnt, mt, n, rg, 0, w.At, w.su.U, w.Bg, w.X1g, nullptr, w.Xg, w.Yg, nullptr, w.iit, nullptr, nullptr, nullptr,
                  (uint32_t*)w.ist, w.state, st);
        if (stage_iters) launch_put_col(cnt, w.iit, gidx, stage_iters, 3, 1, 0u, st);
        if (status) launch_put_col(cnt, w.ist, gidx, (int*)status, 1, 0, ACE_ST_NO_OPT, st);
        launch_put_col(cnt, w.ist, gidx, w.st2, 1, 0, 0u, st);   // ACE_ST_CONVERGED: the last stage a realisation ran
        launch_move_rows(cnt, 2LL * n, w.Xg, w.X2, gidx, true, st);
        launch_move_rows(cnt, 2LL * mt, w.Yg, w.Y2, gidx, true, st);
        ACE_LAUNCHED("minl2 stages");
    }
    // ---- :42-57: the quality on the test rows (NaN without test rows: no refinement), the refinement on the full A
    launch_quality(n, mte, batch, w.Ate, w.X2, w.Bte, w.q, st);
    std::vector<double> q(batch);
    ACE_HIP(read_back(q.data(), w.q, sizeof(double) * (size_t)batch, st));
    if (quality) ACE_HIP(hipMemcpyAsync(quality, w.q, sizeof(double) * (size_t)batch, hipMemcpyDeviceToDevice, st));
    ACE_HIP(hipMemcpyAsync(w.X3, w.X2, 16 * (size_t)batch * n, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ml_pad_y_kernel, dim3(batch), dim3(256), 0, st, m, mt, (const d2*)w.Y2, (d2*)w.Y3);
    std::vector<int> sel;
    for (int b = 0; b < batch; ++b)
        if (q[b] > 0.6) sel.push_back(b);
    if (!sel.empty()) {
        const int cnt = (int)sel.size();
        ACE_TRY(ml_setup(m, n, w.An, w.su, st));
        ACE_HIP(upload(w.gidx, sel.data(), sizeof(int) * (size_t)cnt, st));
        hipLaunchKernelGGL(ml_gather_kernel, dim3(cnt), dim3(256), 0, st, (long long)m, w.Bn, (long long)m, w.Bg, w.gidx);
        hipLaunchKernelGGL(ml_gather_kernel, dim3(cnt), dim3(256), 0, st, 2LL * n, w.X2, 2LL * n, w.X0g, w.gidx);
        ml_launch(cfg, cnt, m, n, 1, 1, w.An, w.su.U, w.Bg, w.X0g, nullptr, w.Xg, w.Yg, nullptr, w.iit, nullptr, nullptr, nullptr,
                  (uint32_t*)w.ist, w.state, st);
        if (stage_iters) launch_put_col(cnt, w.iit, w.gidx, stage_iters, 3, 2, 0u, st);
        launch_move_rows(cnt, 2LL * n, w.Xg, w.X3, w.gidx, true, st);
        launch_move_rows(cnt, 2LL * m, w.Yg, w.Y3, w.gidx, true, st);
        if (status) launch_put_col(cnt, w.ist, w.gidx, (int*)status, 1, 0, ACE_ST_NO_OPT, st);
        launch_put_col(cnt, w.ist, w.gidx, w.st2, 1, 0, 0u, st);   // the refinement's stop test replaces stage 2's
    }
    if (status) launch_put_col(batch, w.st2, nullptr, (int*)status, 1, 0, ACE_ST_CONVERGED, st);
    // ---- :51-63: rollback at similarity < 0.6, X and Y scaled by B_norm / A_norm
    launch_finish(n, m, mt, batch, w.q, w.X3, w.Y3, w.X2, w.Y2, w.anorm, w.bnorm, X, Y, status, st);
    ACE_LAUNCHED("minl2 refinement");
    return ACE_OK;
}

}  // namespace

size_t minl2_request_bytes(int) { return 0; }   // minl2_kernel takes no dynamic LDS

}  // namespace ace

using namespace ace;

extern "C" void ace_minl2_cfg_default(ace_minl2_cfg* cfg) {
    if (!cfg) return;
    cfg->r = 20;
    cfg->maxiter = 500;
    cfg->train_seed = 0;
    cfg->reserved = 0;
    cfg->mu0 = 1e-3;
    cfg->rho = 1.03;
    cfg->cc_frac = 0.95;
    cfg->tol_rel = 1e-4;
    cfg->tol_abs = 1e-8;
}

extern "C" size_t ace_minl2_workspace_size(int batch, int m, int n, int r) {
    if (batch < 1 || m < 1 || m > ML_MMAX || n < 1 || n > ML_NMAX || r < 1 || r > ML_RMAX) return 0;
    return ml_ws_bytes(batch, m, n, r);
}

extern "C" int ace_minl2_admm_batch(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int scale_by_row,
                                    const double* A, const double* B, const double* X0, const int32_t* rcols, double* X,
                                    double* Y, double* Xall, int32_t* iters, int32_t* objcol, double* opt_obj, double* mu,
                                    uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(ml_check_stage(cfg, batch, m, n, r, scale_by_row, A, B, X0, X, Y));
    const size_t need = ml_ws_bytes(batch, m, n, r);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "minl2: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    Carver cv{(char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255)};
    MlSetup su;
    ml_carve_setup(cv, m, n, &su);
    d2* const ws = cv.take<d2>(sizeof(d2) * ml_groups(batch, r) * ml_group_elems(m, n));
    ACE_TRY(ml_setup(m, n, A, su, st));
    ml_launch(cfg, batch, m, n, r, scale_by_row, A, su.U, B, X0, rcols, X, Y, Xall, iters, objcol, opt_obj, mu, status, ws, st);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_minl2_admm_host(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int scale_by_row,
                                   const double* A, const double* B, const double* X0, const int32_t* rcols, double* X,
                                   double* Y, double* Xall, int32_t* iters, int32_t* objcol, double* opt_obj, double* mu,
                                   uint32_t* status) {
    g_err.clear();
    ACE_TRY(ml_check_stage(cfg, batch, m, n, r, scale_by_row, A, B, X0, X, Y));
    const size_t Bn = batch, ro = scale_by_row ? r : 1, wsb = ml_ws_bytes(batch, m, n, r);
    DevScope dev;
    double *dA, *dB, *dX0, *dX, *dY, *dXall = nullptr, *dobj = nullptr, *dmu = nullptr;
    int32_t *drc = nullptr, *dit = nullptr, *doc = nullptr;
    uint32_t* dst = nullptr;
    char* dws;
    ACE_TRY(dev.put(&dA, A, 2 * (size_t)m * n));
    ACE_TRY(dev.put(&dB, B, Bn * m));
    ACE_TRY(dev.put(&dX0, X0, 2 * Bn * r * n));
    if (rcols) ACE_TRY(dev.put(&drc, rcols, Bn));
    ACE_TRY(dev.alloc(&dX, 2 * Bn * ro * n));
    ACE_TRY(dev.alloc(&dY, 2 * Bn * ro * m));
    if (Xall) ACE_TRY(dev.alloc(&dXall, 2 * Bn * r * n));
    if (iters) ACE_TRY(dev.alloc(&dit, Bn));
    if (objcol) ACE_TRY(dev.alloc(&doc, Bn));
    if (opt_obj) ACE_TRY(dev.alloc(&dobj, Bn));
    if (mu) ACE_TRY(dev.alloc(&dmu, Bn));
    if (status) ACE_TRY(dev.alloc(&dst, Bn));
    ACE_TRY(dev.alloc(&dws, wsb));
    ACE_TRY(ace_minl2_admm_batch(cfg, batch, m, n, r, scale_by_row, dA, dB, dX0, drc, dX, dY, dXall, dit, doc, dobj, dmu,
                                 dst, dws, wsb, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(X, dX, 2 * Bn * ro * n));
    ACE_TRY(dev.get(Y, dY, 2 * Bn * ro * m));
    ACE_TRY(dev.get(Xall, dXall, 2 * Bn * r * n));
    ACE_TRY(dev.get(iters, dit, Bn));
    ACE_TRY(dev.get(objcol, doc, Bn));
    ACE_TRY(dev.get(opt_obj, dobj, Bn));
    ACE_TRY(dev.get(mu, dmu, Bn));
    return dev.get(status, dst, Bn);
}

extern "C" size_t ace_minl2_solve_workspace_size(const ace_minl2_cfg* cfg, int batch, int m, int n) {
    MlDims d;
    const std::string keep = g_err;
    if (ml_dims(cfg, batch, m, n, &d)) {
        g_err = keep;
        return 0;
    }
    return ml_solve_bytes(d);
}

extern "C" int ace_minl2_solve_batch(const ace_minl2_cfg* cfg, int batch, int m, int n, const double* A, const double* B,
                                     const int32_t* train_idx_host, double* X, double* Y, double* quality,
                                     int32_t* stage_iters, int32_t* r_used, uint32_t* status, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    g_err.clear();
    MlDims d;
    ACE_TRY(ml_dims(cfg, batch, m, n, &d));
    if (!A || !B || !X || !Y) return fail(ACE_ERR_ARG, "minl2: NULL %s", !A ? "A" : !B ? "B" : !X ? "X" : "Y");
    std::vector<int> rows;
    ACE_TRY(ml_partition(cfg, d, train_idx_host, &rows));
    const size_t need = ml_solve_bytes(d);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "minl2: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    Carver cv{(char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255)};
    MlSolveWs w;
    ml_carve_solve(cv, d, &w);
    return ml_solve(cfg, d, rows, A, B, X, Y, quality, stage_iters, r_used, status, w, (hipStream_t)stream);
}

extern "C" int ace_minl2_solve_host(const ace_minl2_cfg* cfg, int batch, int m, int n, const double* A, const double* B,
                                    const int32_t* train_idx, double* X, double* Y, double* quality, int32_t* stage_iters,
                                    int32_t* r_used, uint32_t* status) {
    g_err.clear();
    MlDims d;
    ACE_TRY(ml_dims(cfg, batch, m, n, &d));
    if (!A || !B || !X || !Y) return fail(ACE_ERR_ARG, "minl2: NULL %s", !A ? "A" : !B ? "B" : !X ? "X" : "Y");
    std::vector<int> rows;
    ACE_TRY(ml_partition(cfg, d, train_idx, &rows));
    const size_t Bn = batch, wsb = ml_solve_bytes(d);
    DevScope dev;
    double *dA, *dB, *dX, *dY, *dq = nullptr;
    int32_t *dit = nullptr, *dru = nullptr;
    uint32_t* dst = nullptr;
    char* dws;
    ACE_TRY(dev.put(&dA, A, 2 * (size_t)m * n));
    ACE_TRY(dev.put(&dB, B, Bn * m));
    ACE_TRY(dev.alloc(&dX, 2 * Bn * n));
    ACE_TRY(dev.alloc(&dY, 2 * Bn * m));
    if (quality) ACE_TRY(dev.alloc(&dq, Bn));
    if (stage_iters) ACE_TRY(dev.alloc(&dit, 3 * Bn));
    if (r_used) ACE_TRY(dev.alloc(&dru, Bn));
    if (status) ACE_TRY(dev.alloc(&dst, Bn));
    ACE_TRY(dev.alloc(&dws, wsb));
    Carver cv{(char*)(((uintptr_t)dws + 255) & ~(uintptr_t)255)};
    MlSolveWs w;
    ml_carve_solve(cv, d, &w);
    ACE_TRY(ml_solve(cfg, d, rows, dA, dB, dX, dY, dq, dit, dru, dst, w, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(X, dX, 2 * Bn * n));
    ACE_TRY(dev.get(Y, dY, 2 * Bn * m));
    ACE_TRY(dev.get(quality, dq, Bn));
    ACE_TRY(dev.get(stage_iters, dit, 3 * Bn));
    ACE_TRY(dev.get(r_used, dru, Bn));
    return dev.get(status, dst, Bn);
}
