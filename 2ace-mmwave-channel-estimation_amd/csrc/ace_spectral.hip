// SpectralInitialize (main/src/my_recovery_algorithms/ADMM_v2/inferLowRankV4_multi.m:561-574)
// for a batch of realisations sharing one train matrix A_t (m_t x n).
//
// The reference forms As^H As (n x n, As = rows of A_t scaled by B_i/||a_i||), calls eig
// and keeps the r largest eigenpairs as X = V diag(sqrt(s)).  Its nonzero spectrum is
// that of the m_t x m_t dual Gram C = D K D (K = A_t A_t^H, shared by the batch;
// D = diag(B_i/||a_i||), per realisation), and As^H u = sqrt(lam) v for an eigenpair
// (lam, u) of C.  So per realisation we need the top-r eigenpairs of a dense m_t x m_t
// Hermitian matrix (243 x 243 at the 32-antenna configuration):
//
//   hetrd_kernel     one work-group per realisation: build C, reduce it to real
//                    symmetric tridiagonal form by Householder reflectors (LAPACK zhetd2,
//                    lower, with full Hermitian storage in global memory so that the
//                    Hermitian matrix-vector product reads rows coalesced); reflector k is
//                    left in row k of C
//   trieig_kernel    one work-group per realisation: the r largest eigenvalues (or, for
//                    PhaseLift's prox_trace, all above a threshold) by Sturm-count
//                    bisection to full precision, then inverse iteration on the
//                    tridiagonal (partial-pivoting LU as LAPACK dgttrf/dgttrs, three
//                    solves), one thread per eigenvalue cluster (relative separation
//                    < 1e-3, as dstein) with the cluster's earlier vectors projected out
//   backxf_kernel    one work-group per realisation: u_k = H_0 H_1 ... H_{m_t-2} z_k,
//                    W_k = D u_k  (few vectors; PhaseLift's prox, which keeps 100-256 of 256,
//                    takes the compact-WY blocked back-transform on the MFMA GEMM instead)
//
// X = A_t^H W is then one MFMA GEMM over batch*r vectors (ace_pipeline.cpp).
// Realisations are processed in chunks so the C matrices of a chunk stay in the L2/MALL.
#include <algorithm>

#include "ace_common.hpp"
#include "ace_pipe.hpp"
#include "ace_host.hpp"

namespace ace {

namespace {
constexpr int SPEC_CHUNK = 256;   // realisations per launch (C = 0.9 MiB each at m_t = 243)
constexpr double kOrtol = 1e-5;   // cluster separation, relative to ||T|| (see trieig_kernel)

// per-realisation scratch layout (units: doubles)
struct SpecLayout {
    long long C, dv, dd, ee, tau, lu, z, lam, cl, misc, stride;
    int kmax, lanes;
    SpecLayout(int mt, int kmax_) {
        kmax = kmax_;
        lanes = kmax <= 64 ? 64 : 256;   // inverse-iteration lanes (one eigenvalue cluster each)
        long long o = 0;
        auto take = [&](long long nd) { long long p = o; o += (nd + 31) & ~31LL; return p; };
        C = take(2LL * mt * mt);
        dv = take(mt);
        dd = take(mt);
        ee = take(mt);
        tau = take(2LL * mt);
        lu = take(6LL * mt * lanes);       // dl, d, du, du2, ipiv, y  (lane-interleaved)
        z = take((long long)kmax * mt);
        lam = take(kmax);
        cl = take(kmax + 1);               // cluster starts (as doubles)
        misc = take(8);                    // [0] k, [1] sum over lam > tau of (lam - tau), [2] side (trieig_kernel)
        stride = o;
    }
};

// 1024 threads per realisation: the Hermitian matrix-vector product and the rank-2 update
// split the trailing matrix's rows four ways (thread = column x row quarter), so each step
// keeps four times as many independent memory streams in flight.
constexpr int HT_THREADS = 1024;
constexpr int HT_COLS = 256;                 // threads per row quarter
constexpr int HT_RB = HT_THREADS / HT_COLS;  // row quarters

// The rank-2 update of step k is applied in the same sweep over the trailing matrix as the
// Hermitian matrix-vector product of step k + 1 (one read and one write per element and step
// instead of a read for the product plus a read and a write for the update).  Row k + 1, which
// the next reflector comes from, takes the pending update on the fly; column k + 1 is never read
// again.  Every element gets the same update expression and every product the same summation
// order as in the two-sweep form.
// rows (PartRows, per-realisation partitions): realisation b's train rows rows[b][0..mt) of the full
// m x m K (leading dimension ldk = m) and of its full B row (ldb = m); null: K is K_t itself (ldk = ldb = mt)
__global__ __launch_bounds__(HT_THREADS) void hetrd_kernel(int mt, const double* Kp, const double* Bt, double* scratch,
                                                           SpecLayout lay, const int* active, const int* rows, int ldk) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (active && !active[b]) return;
    extern __shared__ double smem[];
    d2* vb[2] = {reinterpret_cast<d2*>(smem), reinterpret_cast<d2*>(smem) + 2 * mt};   // reflector / x
    d2* wb[2] = {vb[0] + mt, vb[1] + mt};                                              // p, w
    double* dvs = reinterpret_cast<double*>(vb[1] + 2 * mt);
    __shared__ double red[16 * 2];
    __shared__ d2 part[HT_RB][HT_COLS];
    __shared__ d2 s_tau, s_scal;
    double* base = scratch + b * lay.stride;
    d2* C = reinterpret_cast<d2*>(base + lay.C);
    const d2* K = reinterpret_cast<const d2*>(Kp);
    double* dd = base + lay.dd;
    double* ee = base + lay.ee;
    d2* taus = reinterpret_cast<d2*>(base + lay.tau);
    const int col = t % HT_COLS, rb = t / HT_COLS;

    if (Kp) {
        const int* rw = rows ? rows + (long long)b * ldk : nullptr;
        const int ld = rows ? ldk : mt;
        auto ri = [&](int i) { return rw ? rw[i] : i; };
        // D = diag(B_i / ||a_i||), ||a_i||^2 = K_ii  (SpectralInitialize :563-567; zero rows stay zero)
        for (int i = t; i < mt; i += HT_THREADS) {
            const double kii = K[(long long)ri(i) * ld + ri(i)].x;
            const double d = kii > 0.0 ? Bt[(long long)b * ld + ri(i)] / sqrt(kii) : 0.0;
            dvs[i] = d;
            base[lay.dv + i] = d;
        }
        __syncthreads();
        // C = D (K + K^H)/2 D, exactly Hermitian (real diagonal)
        for (long long e = t; e < (long long)mt * mt; e += HT_THREADS) {
            const int i = (int)(e / mt), j = (int)(e % mt);
            const d2 kij = K[(long long)ri(i) * ld + ri(j)], kji = K[(long long)ri(j) * ld + ri(i)];
            const double s = dvs[i] * dvs[j];
            C[e] = i == j ? make_double2(s * kij.x, 0.0)
                          : make_double2(0.5 * s * (kij.x + kji.x), 0.5 * s * (kij.y - kji.y));
        }
    }
    __syncthreads();

    bool pend = false;   // the update of step k - 1 (pv, pw; index 0 = row k) is not yet applied
    int cur = 0;
    for (int k = 0; k + 1 < mt; ++k) {
        const int L = mt - k - 1;
        d2 *v = vb[cur], *w = wb[cur];
        const d2 *pv = vb[1 - cur], *pw = wb[1 - cur];
        const long long r0 = (long long)(k + 1) * mt + (k + 1);   // C22 origin
        // x = C(k+1:m, k) = conj(C(k, k+1:m)), with the pending update
        double s1[1] = {0.0};
        for (int i = t; i < L; i += HT_THREADS) {
            d2 c = C[(long long)k * mt + k + 1 + i];
            if (pend) {
                const d2 cwj = make_double2(pw[1 + i].x, -pw[1 + i].y), cvj = make_double2(pv[1 + i].x, -pv[1 + i].y);
                c = csub(c, cadd(cmul(pv[0], cwj), cmul(pw[0], cvj)));
            }
            v[i] = make_double2(c.x, -c.y);
            if (i > 0) s1[0] += cabs2(c);
        }
        block_sum<1>(s1, red);
        if (t == 0) {  // zlarfg
            const d2 alpha = v[0];
            const double xn2 = s1[0];
            d2 tau = make_double2(0.0, 0.0), scal = make_double2(0.0, 0.0);
            double beta = alpha.x;
            if (!(xn2 == 0.0 && alpha.y == 0.0)) {
                beta = -copysign(sqrt(alpha.x * alpha.x + alpha.y * alpha.y + xn2), alpha.x);
                tau = make_double2((beta - alpha.x) / beta, -alpha.y / beta);
                const d2 den = make_double2(alpha.x - beta, alpha.y);      // scal = 1 / (alpha - beta)
                const double dn = 1.0 / cabs2(den);
                scal = make_double2(den.x * dn, -den.y * dn);
            }
            s_tau = tau;
            s_scal = scal;
            ee[k] = beta;
            d2 ckk = C[(long long)k * mt + k];
            if (pend) {
                const d2 cw0 = make_double2(pw[0].x, -pw[0].y), cv0 = make_double2(pv[0].x, -pv[0].y);
                ckk = csub(ckk, cadd(cmul(pv[0], cw0), cmul(pw[0], cv0)));
            }
            dd[k] = ckk.x;
            taus[k] = tau;
        }
        __syncthreads();
        const d2 tau = s_tau;
        const bool refl = !(tau.x == 0.0 && tau.y == 0.0);   // H = I otherwise (uniform branch)
        if (refl) {
            const d2 scal = s_scal;
            for (int i = t; i < L; i += HT_THREADS) {
                const d2 vi = i == 0 ? make_double2(1.0, 0.0) : cmul(v[i], scal);
                v[i] = vi;
                C[(long long)k * mt + k + 1 + i] = vi;  // reflector k kept in row k (for the back transform)
            }
            __syncthreads();
        }
        if (!refl && !pend) continue;
        // one sweep over C22: the pending update (rows / columns 1.. of step k - 1), and
        // p = tau C22 v: p_i = tau sum_j conj(C22[j][i]) v_j (thread (col, rb) sums rows j = rb, rb + 4, ...)
        for (int i0 = 0; i0 < L; i0 += HT_COLS) {
            const int i = i0 + col;
            double ar = 0.0, ai = 0.0;
            if (i < L) {
                d2* cc = C + r0 + i;
                if (pend) {
                    const d2 cwj = make_double2(pw[1 + i].x, -pw[1 + i].y), cvj = make_double2(pv[1 + i].x, -pv[1 + i].y);
                    if (refl) {
#pragma unroll 4
                        for (int j = rb; j < L; j += HT_RB) {
                            d2 c = cc[(long long)j * mt];
                            c = csub(c, cadd(cmul(pv[1 + j], cwj), cmul(pw[1 + j], cvj)));
                            cc[(long long)j * mt] = c;
                            const d2 vj = v[j];
                            ar += c.x * vj.x + c.y * vj.y;
                            ai += c.x * vj.y - c.y * vj.x;
                        }
                    } else {
#pragma unroll 4
                        for (int j = rb; j < L; j += HT_RB) {
                            d2 c = cc[(long long)j * mt];
                            c = csub(c, cadd(cmul(pv[1 + j], cwj), cmul(pw[1 + j], cvj)));
                            cc[(long long)j * mt] = c;
                        }
                    }
                } else {
#pragma unroll 4
                    for (int j = rb; j < L; j += HT_RB) {
                        const d2 c = cc[(long long)j * mt], vj = v[j];
                        ar += c.x * vj.x + c.y * vj.y;
                        ai += c.x * vj.y - c.y * vj.x;
                    }
                }
            }
            if (refl) {
                part[rb][col] = make_double2(ar, ai);
                __syncthreads();
                if (rb == 0 && i < L) {
                    d2 acc = part[0][col];
#pragma unroll
                    for (int q = 1; q < HT_RB; ++q) acc = cadd(acc, part[q][col]);
                    w[i] = cmul(tau, acc);
                }
                __syncthreads();
            }
        }
        pend = refl;
        if (!refl) {
            __syncthreads();
            continue;
        }
        double s2[2] = {0.0, 0.0};  // p^H v
        for (int i = t; i < L; i += HT_THREADS) {
            const d2 q = cmulc(w[i], v[i]);
            s2[0] += q.x;
            s2[1] += q.y;
        }
        block_sum<2>(s2, red);
        const d2 alpha2 = cscale(cmul(tau, make_double2(s2[0], s2[1])), -0.5);
        for (int i = t; i < L; i += HT_THREADS) w[i] = cadd(w[i], cmul(alpha2, v[i]));
        __syncthreads();
        cur = 1 - cur;   // (v, w) of step k become the pending update of step k + 1
    }
    __syncthreads();
    if (t == 0) {
        d2 c = C[(long long)(mt - 1) * mt + mt - 1];
        if (pend) {
            const d2 *pv = vb[1 - cur], *pw = wb[1 - cur];
            const d2 cw0 = make_double2(pw[0].x, -pw[0].y), cv0 = make_double2(pv[0].x, -pv[0].y);
            c = csub(c, cadd(cmul(pv[0], cw0), cmul(pw[0], cv0)));
        }
        dd[mt - 1] = c.x;
        ee[mt - 1] = 0.0;
    }
}
size_t hetrd_lds(int mt) { return (size_t)mt * (4 * 16 + 8); }
bool hetrd_lds_ok(int mt) {
    const size_t need = hetrd_lds(mt);
    return need <= 64 * 1024 || need <= lds_dyn_budget(reinterpret_cast<const void*>(&hetrd_kernel));
}

// C = D (K + K^H)/2 D and dv into the scratch (hetrd_kernel's own prologue as a kernel of its own), for
// the blocked reduction of the spectral initialisation: the same expressions per element
__global__ __launch_bounds__(256) void spec_form_c_kernel(int mt, const double* Kp, const double* Bt, double* scratch,
                                                           SpecLayout lay, const int* rows, int ldk) {
    const int b = blockIdx.x, t = threadIdx.x;
    extern __shared__ double dvs[];   // [mt]
    double* base = scratch + b * lay.stride;
    d2* C = reinterpret_cast<d2*>(base + lay.C);
    const d2* K = reinterpret_cast<const d2*>(Kp);
    const int* rw = rows ? rows + (long long)b * ldk : nullptr;
    const int ld = rows ? ldk : mt;
    auto ri = [&](int i) { return rw ? rw[i] : i; };
    for (int i = t; i < mt; i += 256) {
        const double kii = K[(long long)ri(i) * ld + ri(i)].x;
        const double d = kii > 0.0 ? Bt[(long long)b * ld + ri(i)] / sqrt(kii) : 0.0;
        dvs[i] = d;
        base[lay.dv + i] = d;
    }
    __syncthreads();
    for (long long e = t; e < (long long)mt * mt; e += 256) {
        const int i = (int)(e / mt), j = (int)(e % mt);
        const d2 kij = K[(long long)ri(i) * ld + ri(j)], kji = K[(long long)ri(j) * ld + ri(i)];
        const double s = dvs[i] * dvs[j];
        C[e] = i == j ? make_double2(s * kij.x, 0.0)
                      : make_double2(0.5 * s * (kij.x + kji.x), 0.5 * s * (kij.y - kji.y));
    }
}

// Blocked form of the same reduction (LAPACK zhetrd / zlatrd) for PhaseLift's prox (C already in the
// scratch): the reflectors of a panel of HB_NB columns are generated against the panel-start matrix plus
// the panel's own rank-2 corrections (V W^H + W V^H held in LDS), so a column's Hermitian product only
// READS the trailing matrix, and the trailing matrix is written once per panel.  Per panel that is
// HB_NB + 2 passes over the trailing matrix instead of hetrd_kernel's 2 HB_NB (read + write per step):
// the kernel is bound by that traffic (the matrices live in the L2 / MALL).  The outputs are hetrd_kernel's:
// d, e, tau and reflector k in row k of C.
// Fixed geometry (r05 A/B measurements; the variants measured and not kept were removed in r06):
// panels of HB_NB = 4 columns in the prox (2 in the spectral initialisation, whose small batches are
// latency-bound), 1024 threads per matrix, the lower triangle only (half the bytes of the full square; row sums
// reduced across each DPP row of 16 lanes), the reductions on DPP with one barrier per block sum, the
// corrections' wave sums for all q side by side, the trailing update by balanced column pairs with HB_TB rows
// per memory round trip.
constexpr int HB_NB = 4;        // panel width (PhaseLift's prox)
constexpr int HB_NB_SPEC = 2;   // panel width of the spectral initialisation
constexpr int HB_THREADS = 1024;   // threads per matrix
constexpr int HB_TB = 4;        // trailing-update rows per memory round trip
constexpr int HB_NW = HB_THREADS / 64;   // waves
__host__ __device__ constexpr int hb_strips(int mt) { return (mt + 63) >> 6; }
size_t hetrd_blk_lds(int mt, int nb = HB_NB) {
    return (size_t)mt * 16 * (2 * nb + 2) + (size_t)hb_strips(mt) * mt * 16 + (size_t)(HB_NW + hb_strips(mt)) * 64 * 16;
}
template <int NB>
__global__ __launch_bounds__(HB_THREADS) void hetrd_blk_kernel(int mt, double* scratch, SpecLayout lay, const int* active) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (active && !active[b]) return;
    extern __shared__ double smem[];
    d2* Vp = reinterpret_cast<d2*>(smem);   // [NB][mt]: the panel's reflectors by absolute row (0 elsewhere)
    d2* Wp = Vp + NB * mt;               // [NB][mt]: their w
    d2* v = Wp + NB * mt;                // current reflector, entry i = row k + 1 + i
    d2* w = v + mt;
    __shared__ double red[16 * 4 * NB];   // (block_sum: 16 waves; the corrections: [q][wave][4])
    d2* rowp = w + mt;                        // [strip][row]: row sums of the lower triangle, per 64-column strip
    d2* colp = rowp + hb_strips(mt) * mt;     // [wave + strip][64]: column sums, per wave and strip
    __shared__ d2 s_tau, s_scal, s_cw[NB], s_cv[NB];
    double* base = scratch + b * lay.stride;
    d2* C = reinterpret_cast<d2*>(base + lay.C);
    double* dd = base + lay.dd;
    double* ee = base + lay.ee;
    d2* taus = reinterpret_cast<d2*>(base + lay.tau);
    auto cj = [](d2 a) { return make_double2(a.x, -a.y); };
    for (int k0 = 0; k0 + 1 < mt; k0 += NB) {
        const int nbp = min(NB, mt - 1 - k0);
        for (int e = t; e < 2 * NB * mt; e += HB_THREADS) Vp[e] = make_double2(0.0, 0.0);
        __syncthreads();
        for (int p = 0; p < nbp; ++p) {
            const int k = k0 + p, L = mt - k - 1;
            // row k of the current matrix: the panel-start C minus the panel's earlier rank-2 updates
            double s1[1] = {0.0};
            for (int i = t; i < L; i += HB_THREADS) {
                const int c = k + 1 + i;
                // column k below the diagonal (the upper triangle is not kept)
                d2 a = C[(long long)c * mt + k];
                for (int q = 0; q < p; ++q)
                    a = csub(a, cadd(cmul(Vp[q * mt + c], cj(Wp[q * mt + k])), cmul(Wp[q * mt + c], cj(Vp[q * mt + k]))));
                v[i] = a;   // x_i = A[k + 1 + i][k]
                if (i > 0) s1[0] += cabs2(a);
            }
            block_sum_dpp1<1>(s1, red);
            if (t == 0) {   // zlarfg
                const d2 alpha = v[0];
                const double xn2 = s1[0];
                d2 tau = make_double2(0.0, 0.0), scal = make_double2(0.0, 0.0);
                double beta = alpha.x;
                if (!(xn2 == 0.0 && alpha.y == 0.0)) {
                    beta = -copysign(sqrt(alpha.x * alpha.x + alpha.y * alpha.y + xn2), alpha.x);
                    tau = make_double2((beta - alpha.x) / beta, -alpha.y / beta);
                    const d2 den = make_double2(alpha.x - beta, alpha.y);
                    const double dn = 1.0 / cabs2(den);
                    scal = make_double2(den.x * dn, -den.y * dn);
                }
                s_tau = tau;
                s_scal = scal;
                ee[k] = beta;
                d2 ckk = C[(long long)k * mt + k];
                for (int q = 0; q < p; ++q)
                    ckk = csub(ckk, cadd(cmul(Vp[q * mt + k], cj(Wp[q * mt + k])), cmul(Wp[q * mt + k], cj(Vp[q * mt + k]))));
                dd[k] = ckk.x;
                taus[k] = tau;
            }
            __syncthreads();
            const d2 tau = s_tau;
            if (tau.x == 0.0 && tau.y == 0.0) continue;   // H = I (uniform): V, W of this column stay 0
            const d2 scal = s_scal;
            for (int i = t; i < L; i += HB_THREADS) {
                const d2 vi = i == 0 ? make_double2(1.0, 0.0) : cmul(v[i], scal);
                v[i] = vi;
                C[(long long)k * mt + k + 1 + i] = vi;   // reflector k kept in row k (for the back transform)
                Vp[p * mt + k + 1 + i] = vi;
            }
            // the panel's corrections to C22 v: s_q = W_q^H v, t_q = V_q^H v (L < 1024: one entry per thread)
            __syncthreads();
            // every q's dot products first, then their wave sums side by side (independent chains)
            if (p > 0) {
                d2 a[NB], c2[NB];
#pragma unroll
                for (int q = 0; q < NB; ++q) a[q] = c2[q] = make_double2(0.0, 0.0);
                for (int i = t; i < L; i += HB_THREADS) {
                    const int r = k + 1 + i;
                    const d2 vi = v[i];
#pragma unroll
                    for (int q = 0; q < NB; ++q)
                        if (q < p) {
                            a[q] = cadd(a[q], cmulc(Wp[q * mt + r], vi));
                            c2[q] = cadd(c2[q], cmulc(Vp[q * mt + r], vi));
                        }
                }
#pragma unroll
                for (int q = 0; q < NB; ++q) {
                    if (q >= p) break;
                    const double a0 = wave_sum_dpp(a[q].x), a1 = wave_sum_dpp(a[q].y), c0 = wave_sum_dpp(c2[q].x),
                                 c1 = wave_sum_dpp(c2[q].y);
                    if ((t & 63) == 0) {
                        red[(q * 16 + (t >> 6)) * 4 + 0] = a0;
                        red[(q * 16 + (t >> 6)) * 4 + 1] = a1;
                        red[(q * 16 + (t >> 6)) * 4 + 2] = c0;
                        red[(q * 16 + (t >> 6)) * 4 + 3] = c1;
                    }
                }
            }
            __syncthreads();
            if (t < p) {   // fixed order over the 16 waves
                double sw0 = 0.0, sw1 = 0.0, sv0 = 0.0, sv1 = 0.0;
                for (int ww = 0; ww < HB_THREADS / 64; ++ww) {
                    const double* r4 = red + (t * 16 + ww) * 4;
                    sw0 += r4[0];
                    sw1 += r4[1];
                    sv0 += r4[2];
                    sv1 += r4[3];
                }
                s_cw[t] = make_double2(sw0, sw1);
                s_cv[t] = make_double2(sv0, sv1);
            }
            __syncthreads();
            // p = tau (C22 v - V s - W t): the sweep only reads C22 (thread (col, rb): rows rb, rb + 4, ...)
            const long long r0 = (long long)(k + 1) * mt + (k + 1);
            // From the lower triangle only: element (j, i), j >= i, adds conj(c) v_j to p_i (column sums) and,
            // for j > i, c v_i to p_j (row sums).  Tasks are 4-row groups of 64-column strips (strip s: columns
            // 64s.., rows 64s..L-1), dealt to the waves in contiguous runs; lane (jr, ic) reads row jr of the
            // group at columns ic + 16q (four 256-B rows per load).  A row's sum over a strip is reduced over
            // the 16 ic lanes; a wave's column sums over its run in a strip over the 4 jr lanes at the end of
            // the run (slot wave + strip: unique, since the runs are contiguous).
            {
                const int ns = hb_strips(L), wv = t >> 6, jr = (t & 63) >> 4, ic = t & 15;
                constexpr int TR = 1;   // rows per lane and task (a task: 4 TR rows of a strip)
                auto ngr = [&](int s) { return (L - 64 * s + 4 * TR - 1) / (4 * TR); };
                int G = 0;
                for (int s = 0; s < ns; ++s) G += ngr(s);
                const int g0 = wv * G / HB_NW, g1 = (wv + 1) * G / HB_NW;
                const d2* C22 = C + r0;
                int s = 0, gb = 0;
                while (s < ns && g0 >= gb + ngr(s)) gb += ngr(s++);
                d2 ca[4];
                auto strip_start = [&]() {
#pragma unroll
                    for (int q = 0; q < 4; ++q) ca[q] = make_double2(0.0, 0.0);
                };
                auto flush = [&]() {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        double x = ca[q].x, y = ca[q].y;
#pragma unroll
                        for (int o = 16; o < 64; o <<= 1) {
                            x += __shfl_xor(x, o, 64);
                            y += __shfl_xor(y, o, 64);
                        }
                        if (jr == 0) colp[(wv + s) * 64 + ic + 16 * q] = make_double2(x, y);
                    }
                };
                if (g0 < g1) strip_start();
                for (int g = g0; g < g1; ++g) {
                    if (g - gb >= ngr(s)) {
                        flush();
                        gb += ngr(s++);
                        strip_start();
                    }
                    d2 c[TR][4];   // the task's loads, all issued before its sums
#pragma unroll
                    for (int h = 0; h < TR; ++h) {
                        const int j = 64 * s + 4 * TR * (g - gb) + jr + 4 * h;
                        const bool jv = j < L;
                        const d2* crow = C22 + (long long)(jv ? j : 0) * mt + 64 * s + ic;
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            c[h][q] = (jv && 64 * s + ic + 16 * q <= j) ? crow[16 * q] : make_double2(0.0, 0.0);
                    }
#pragma unroll
                    for (int h = 0; h < TR; ++h) {
                        const int j = 64 * s + 4 * TR * (g - gb) + jr + 4 * h;
                        const bool jv = j < L;
                        const d2 vj = jv ? v[j] : make_double2(0.0, 0.0);
                        double rx = 0.0, ry = 0.0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            ca[q].x += c[h][q].x * vj.x + c[h][q].y * vj.y;
                            ca[q].y += c[h][q].x * vj.y - c[h][q].y * vj.x;
                            if (64 * s + ic + 16 * q < j) {   // (then i < L: v[i] is live)
                                const d2 vi = v[64 * s + ic + 16 * q];
                                rx += c[h][q].x * vi.x - c[h][q].y * vi.y;
                                ry += c[h][q].x * vi.y + c[h][q].y * vi.x;
                            }
                        }
                        rx = bsum16(rx);   // over the 16 ic lanes: one DPP row
                        ry = bsum16(ry);
                        if (ic == 0 && jv) rowp[s * mt + j] = make_double2(rx, ry);
                    }
                }
                if (g0 < g1) flush();
                __syncthreads();
                for (int i = t; i < L; i += HB_THREADS) {
                    const int si = i >> 6;
                    int bs = 0;
                    for (int q = 0; q < si; ++q) bs += ngr(q);
                    const int be = bs + ngr(si);
                    d2 acc = make_double2(0.0, 0.0);
                    for (int ww = 0; ww < HB_NW; ++ww)   // the runs that cover strip si, in wave order
                        if (ww * G / HB_NW < be && (ww + 1) * G / HB_NW > bs && ww * G / HB_NW < (ww + 1) * G / HB_NW)
                            acc = cadd(acc, colp[(ww + si) * 64 + (i & 63)]);
                    for (int q = 0; q <= si; ++q) acc = cadd(acc, rowp[q * mt + i]);
                    const int r = k + 1 + i;
                    for (int q = 0; q < p; ++q)
                        acc = csub(acc, cadd(cmul(Vp[q * mt + r], s_cw[q]), cmul(Wp[q * mt + r], s_cv[q])));
                    w[i] = cmul(tau, acc);
                }
                __syncthreads();
            }
            // w = p - (tau / 2) (p^H v) v
            double s2[2] = {0.0, 0.0};
            for (int i = t; i < L; i += HB_THREADS) {
                const d2 q = cmulc(w[i], v[i]);
                s2[0] += q.x;
                s2[1] += q.y;
            }
            block_sum_dpp1<2>(s2, red);
            const d2 alpha2 = cscale(cmul(tau, make_double2(s2[0], s2[1])), -0.5);
            for (int i = t; i < L; i += HB_THREADS) {
                const d2 wi = cadd(w[i], cmul(alpha2, v[i]));
                Wp[p * mt + k + 1 + i] = wi;
            }
            __syncthreads();
        }
        // the trailing matrix past the panel: C -= sum_q (V_q W_q^H + W_q V_q^H), one read and write
        const int kn = k0 + nbp, L2 = mt - kn;
        // the lower triangle's columns in pairs (i, L2 - 1 - i): every thread of a pair's HB_THREADS / 128 row groups
        // updates L2 + 1 entries over the two columns (one column from 0 would do L2 alone)
        {
            constexpr int PRB = HB_THREADS / 128;
            const int np = (L2 + 1) >> 1, pp = t % 128, prb = t / 128;
            for (int p0 = 0; p0 < np; p0 += 128) {
                const int pi = p0 + pp;
                if (pi >= np) continue;
#pragma unroll 1
                for (int side = 0; side < 2; ++side) {
                    const int i = side ? L2 - 1 - pi : pi;
                    if (side && i == pi) break;   // the middle column of an odd order
                    const int ci = kn + i;
                    d2 vq[NB], wq[NB];
#pragma unroll
                    for (int q = 0; q < NB; ++q) {
                        vq[q] = cj(Vp[q * mt + ci]);
                        wq[q] = cj(Wp[q * mt + ci]);
                    }
                    const int js = i + (((prb - i) % PRB) + PRB) % PRB;
                    for (int j0 = js; j0 < L2; j0 += HB_TB * PRB) {
                        d2 cb[HB_TB];
#pragma unroll
                        for (int u = 0; u < HB_TB; ++u) {
                            const int j = j0 + u * PRB;
                            cb[u] = j < L2 ? C[(long long)(kn + j) * mt + ci] : make_double2(0.0, 0.0);
                        }
#pragma unroll
                        for (int u = 0; u < HB_TB; ++u) {
                            const int j = j0 + u * PRB;
                            if (j >= L2) break;
                            const int rj = kn + j;
                            d2 c = cb[u];
#pragma unroll
                            for (int q = 0; q < NB; ++q)
                                c = csub(c, cadd(cmul(Vp[q * mt + rj], wq[q]), cmul(Wp[q * mt + rj], vq[q])));
                            C[(long long)rj * mt + ci] = c;
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) {
        dd[mt - 1] = C[(long long)(mt - 1) * mt + mt - 1].x;
        ee[mt - 1] = 0.0;
    }
}

// Sturm count: number of eigenvalues of the tridiagonal (d, e) below x.
__device__ __forceinline__ int sturm_count(const double* d, const double* e, int n, double x, double pivmin) {
    int cnt = 0;
    double q = d[0] - x;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
    for (int i = 1; i < n; ++i) {
        q = d[i] - x - e[i - 1] * e[i - 1] / q;
        if (fabs(q) < pivmin) q = -pivmin;
        cnt += q < 0.0;
    }
    return cnt;
}
// Bisection stops at LAPACK dstebz's width max(2 ulp |lambda|, ulp ||T||, pivmin) (its default ABSTOL <= 0); a
// relative-only test refined eigenvalues far below ||T|| to their own ulp, ~20 rounds more (r05).
// TE_GRID: one shared round of Sturm counts at TE_GRID + 1 even points first (r05: PhaseLift 69.4 -> 69.9 rec/s)
constexpr int TE_GRID = 512;
// inverse-iteration solves per eigenvector: with the eigenvalue to full precision, one solve leaves the other
// eigenvectors at <= eps ||T|| / gap of the vector (gap >= kOrtol ||T||, closer ones are a cluster and projected
// out), the second squares that (r05: 3 -> 2, PhaseLift 67.6 -> 69.3 rec/s; LAPACK dstein stops 2 solves after
// its growth test passes)
constexpr int TE_SWEEPS = 2;
constexpr int TE_PF = 8;   // rows of the LU solves' loads issued ahead of their dependent chain
// 1 / x from the v_rcp_f64 seed and two Newton steps (~1 ulp; x finite and nonzero here)
__device__ __forceinline__ double rcp_nr(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(y, fma(-x, y, 1.0), y);
    y = fma(y, fma(-x, y, 1.0), y);
    return y;
}
// Sturm counts at two points at once (two independent chains: the bisection's trisection probes), with
// e2 = e^2 precomputed and the reciprocal instead of the IEEE division on the dependent chain
__device__ __forceinline__ void sturm_count2(const double* d, const double* e2, int n, double x0, double x1,
                                             double pivmin, int& c0, int& c1) {
    double q0 = d[0] - x0, q1 = d[0] - x1;
    if (fabs(q0) < pivmin) q0 = -pivmin;
    if (fabs(q1) < pivmin) q1 = -pivmin;
    int n0 = q0 < 0.0, n1 = q1 < 0.0;
    for (int i = 1; i < n; ++i) {
        const double di = d[i], ei = e2[i - 1];
        q0 = (di - x0) - ei * rcp_nr(q0);
        q1 = (di - x1) - ei * rcp_nr(q1);
        if (fabs(q0) < pivmin) q0 = -pivmin;
        if (fabs(q1) < pivmin) q1 = -pivmin;
        n0 += q0 < 0.0;
        n1 += q1 < 0.0;
    }
    c0 = n0;
    c1 = n1;
}

// The eigenvector of an isolated eigenvalue lq (no other within kOrtol ||T||) by one twisted factorization
// (Fernando; Parlett & Dhillon, the core of LAPACK dstemr's dlar1v, here on T - lq I itself):
//   T - lq I = L+ D+ L+^T  (top down: D+_0 = d_0 - lq, L_i = e_i / D+_i, D+_{i+1} = d_{i+1} - lq - L_i e_i)
//            = U- D- U-^T  (bottom up: D-_{n-1} = d_{n-1} - lq, U_i = e_i / D-_{i+1}, D-_i = d_i - lq - U_i e_i),
// gamma_k = D+_k + D-_k - (d_k - lq), r = argmin |gamma_k|, z_r = 1, z_i = -L_i z_{i+1} (i < r),
// z_{i+1} = -U_i z_i (i >= r), normalised.  It is the inverse-iteration step from the best unit start vector e_r
// ((T - lq I) z = gamma_r e_r), in three passes over the row with two stored arrays instead of dgttrf's five and two
// solves (the LU arrays are the path's HBM traffic).  Near-zero pivots are moved to +-tiny as in dlagts.  Returns
// false (nothing written that the caller keeps) if the vector is not finite: the caller's inverse iteration then
// runs.
template <class At>
__device__ bool twisted_vector(const double* d, const double* e, int mt, double lq, double tiny, double* zq, At at) {
    auto guard = [&](double x) { return fabs(x) < tiny ? (x < 0.0 ? -tiny : tiny) : x; };
    double Dp = guard(d[0] - lq);
    for (int i = 0; i + 1 < mt; ++i) {   // top down: D+ (array 1), L (array 0)
        const double Li = e[i] / Dp;
        at(1, i) = Dp;
        at(0, i) = Li;
        Dp = guard(d[i + 1] - lq - Li * e[i]);
    }
    at(1, mt - 1) = Dp;
    // bottom up: U (array 2), gamma against the stored D+ (loads issued TE_PF rows ahead of the chain)
    double Dm = guard(d[mt - 1] - lq), best = fabs(Dp);
    int r = mt - 1;
    for (int i0 = mt - 2; i0 >= 0; i0 -= TE_PF) {
        double dpv[TE_PF];
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) dpv[u] = at(1, max(i0 - u, 0));
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) {
            const int i = i0 - u;
            if (i < 0) break;
            const double Ui = e[i] / Dm;
            at(2, i) = Ui;
            const double dl = d[i] - lq;
            Dm = guard(dl - Ui * e[i]);
            const double g = fabs(dpv[u] + Dm - dl);
            if (g < best) {
                best = g;
                r = i;
            }
        }
    }
    // z outward from r (loads ahead of the chain), then normalised in place
    double nrm = 1.0, z = 1.0;
    zq[r] = 1.0;
    for (int i0 = r - 1; i0 >= 0; i0 -= TE_PF) {
        double lv[TE_PF];
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) lv[u] = at(0, max(i0 - u, 0));
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) {
            const int i = i0 - u;
            if (i < 0) break;
            z = -lv[u] * z;
            zq[i] = z;
            nrm += z * z;
        }
    }
    z = 1.0;
    for (int i0 = r; i0 + 1 < mt; i0 += TE_PF) {
        double uv[TE_PF];
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) uv[u] = at(2, min(i0 + u, mt - 2));
#pragma unroll
        for (int u = 0; u < TE_PF; ++u) {
            const int i = i0 + u;
            if (i + 1 >= mt) break;
            z = -uv[u] * z;
            zq[i + 1] = z;
            nrm += z * z;
        }
    }
    if (!(nrm < INFINITY)) return false;   // (overflow or NaN: the caller's inverse iteration)
    const double inv = 1.0 / sqrt(nrm);
    constexpr int TE_CP = 32;
    for (int i0 = 0; i0 < mt; i0 += TE_CP) {
        double tv[TE_CP];
#pragma unroll
        for (int u = 0; u < TE_CP; ++u) tv[u] = zq[min(i0 + u, mt - 1)];
#pragma unroll
        for (int u = 0; u < TE_CP; ++u)
            if (i0 + u < mt) zq[i0 + u] = tv[u] * inv;
    }
    return true;
}

// dynamic LDS of trieig_kernel: d, e, e^2 and the eigenvalues (k <= mt), mt doubles each
size_t trieig_lds(int mt) { return (size_t)mt * 32; }

// A small cluster whose eigenvalues are still apart by TE_TW_GAP ||T|| or more: each vector by the twisted
// factorization, then orthogonalised against the cluster's earlier ones (modified Gram-Schmidt).  A vector's error is
// a rotation inside the cluster of angle ~ eps ||T|| / gap, which moves the residual and the prox's projector
// sum (lam - tau) v v^H only by ~ eps ||T|| (the rotation times the eigenvalue difference).  Closer eigenvalues (or a
// non-finite vector) return false: the caller's inverse iteration with distinct start vectors runs.
constexpr int TE_TW_CL = 4;
constexpr double TE_TW_GAP = 1e-9;
template <class At>
__device__ bool twisted_cluster(const double* d, const double* e, int mt, const double* slam, int q0, int q1, double tn,
                                double tiny, double* Z, At at) {
    for (int q = q0 + 1; q < q1; ++q)
        if (fabs(slam[q - 1] - slam[q]) < TE_TW_GAP * tn) return false;
    for (int q = q0; q < q1; ++q) {
        double* zq = Z + (long long)q * mt;
        if (!twisted_vector(d, e, mt, slam[q], tiny, zq, at)) return false;
        for (int p = q0; p < q; ++p) {
            const double* zp = Z + (long long)p * mt;
            double sp = 0.0;
            for (int i = 0; i < mt; ++i) sp += zp[i] * zq[i];
            for (int i = 0; i < mt; ++i) zq[i] -= sp * zp[i];
        }
        if (q > q0) {
            double nrm = 0.0;
            for (int i = 0; i < mt; ++i) nrm += zq[i] * zq[i];
            if (!(nrm > 0.0 && nrm < INFINITY)) return false;
            const double inv = 1.0 / sqrt(nrm);
            for (int i = 0; i < mt; ++i) zq[i] *= inv;
        }
    }
    return true;
}

// Eigenpairs of the tridiagonal (d, e) (one work-group per realisation): the kmax largest
// (tau == nullptr) or all eigenvalues above tau[b] (prox_trace, at most kmax), descending.
// Bisection by Sturm counts to full precision; inverse iteration with the partial-pivoting
// LU of LAPACK dgttrf/dgttrs, TE_SWEEPS solves, one thread per eigenvalue cluster with the
// cluster's earlier vectors projected out after every solve (as dstein).  Clusters are runs of
// eigenvalues closer than kOrtol ||T||.  LAPACK's dstein uses 1e-3; on PhaseLift's prox inputs
// that chains up to ~100 eigenvalues into one sequential cluster, while at 1e-5 the largest
// cluster has two members.  Inverse-iteration vectors of eigenvalues separated by more than
// kOrtol ||T|| are orthogonal to ~eps / kOrtol (2e-11) without projection.  Writes z[k][mt], lam[k], misc = {k, sum(lam - tau)}.
// side_ok (the prox, kmax = mt): when more than half of the eigenvalues lie above tau, the vectors of the ones at
// or below it are computed instead (ascending), misc[2] = 1: prox_trace's shrink is then
// X = (W - tau I) + sum_{lam <= tau} (tau - lam) v v^H (the same matrix; PhaseLift's take_z adds W - tau I), and
// misc[1] = sum_{lam > tau} (lam - tau) = (trace T - mt tau) - sum_{lam <= tau} (lam - tau).
__global__ __launch_bounds__(256) void trieig_kernel(int mt, const double* tau_p, double* scratch, SpecLayout lay,
                                                     int* status, int status_off, const int* active, int side_ok) {
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (active && !active[b]) return;
#ifdef ACE_H2_STAMPS
    unsigned long long st_ph[4] = {0, 0, 0, 0}, st_t = __builtin_amdgcn_s_memrealtime(), st_t0 = st_t;
    auto stamp = [&](int ph) {
        const unsigned long long n = __builtin_amdgcn_s_memrealtime();
        st_ph[ph] += n - st_t;
        st_t = n;
    };
#else
    auto stamp = [](int) {};
#endif
    extern __shared__ double smem[];
    double* d = smem;
    double* e = smem + mt;
    double* e2 = smem + 2 * mt;
    double* slam = smem + 3 * mt;   // (the eigenvalues again, for the serial cluster scan)
    __shared__ double red[3 * 4];
    __shared__ int s_k, s_ncl;
    double* base = scratch + b * lay.stride;
    for (int i = t; i < mt; i += 256) {
        d[i] = base[lay.dd + i];
        e[i] = base[lay.ee + i];
        e2[i] = e[i] * e[i];
    }
    __syncthreads();
    // Gershgorin interval and pivmin (LAPACK dstebz)
    double gl = INFINITY, gu = -INFINITY, emax = 0.0;
    for (int i = t; i < mt; i += 256) {
        const double a = i > 0 ? fabs(e[i - 1]) : 0.0, c = i + 1 < mt ? fabs(e[i]) : 0.0;
        gl = fmin(gl, d[i] - a - c);
        gu = fmax(gu, d[i] + a + c);
        if (i + 1 < mt) emax = fmax(emax, e[i] * e[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        gl = fmin(gl, __shfl_xor(gl, o, 64));
        gu = fmax(gu, __shfl_xor(gu, o, 64));
        emax = fmax(emax, __shfl_xor(emax, o, 64));
    }
    if (lane == 0) { red[wv] = gl; red[4 + wv] = gu; red[8 + wv] = emax; }
    __syncthreads();
    gl = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    gu = fmax(fmax(red[4], red[5]), fmax(red[6], red[7]));
    emax = fmax(fmax(red[8], red[9]), fmax(red[10], red[11]));
    const double eps = 2.220446049250313e-16;
    const double tn = fmax(fabs(gl), fabs(gu));
    const double pivmin = 2.2250738585072014e-308 * fmax(1.0, emax);
    gl -= 2.0 * tn * eps * mt;
    gu += 2.0 * tn * eps * mt;
    const double tau = tau_p ? tau_p[status_off + b] : 0.0;
    __shared__ int s_side;
    if (t == 0) {
        int k = lay.kmax < mt ? lay.kmax : mt, side = 0;
        if (tau_p) {  // eigenvalues strictly above tau (prox_trace keeps s = lam - tau > 0)
            const int kk = mt - sturm_count(d, e, mt, tau, pivmin);
            if (kk > k && status) atomicOr(&status[status_off + b], (int)ACE_ST_EIG_NOCONV);
            k = kk < k ? kk : k;
            if (side_ok && 2 * kk > mt) {
                side = 1;
                k = mt - kk;
            }
        }
        s_k = k;
        s_side = side;
    }
    __syncthreads();
    int k = s_k, side = s_side;
    double* lam = base + lay.lam;
    // one shared round first: Sturm counts at TE_GRID + 1 even points of [gl, gu] (two per thread), so that
    // every eigenvalue starts from its grid cell instead of the whole interval (log3(TE_GRID) rounds fewer)
    __shared__ int gcnt[TE_GRID + 1];
    const double gh = (gu - gl) / TE_GRID;
    for (int g = 1 + 2 * t; g <= TE_GRID; g += 512) {
        int ca, cb;
        sturm_count2(d, e2, mt, gl + g * gh, gl + min(g + 1, TE_GRID) * gh, pivmin, ca, cb);
        gcnt[g] = ca;
        if (g + 1 <= TE_GRID) gcnt[g + 1] = cb;
    }
    if (t == 0) gcnt[0] = 0;
    __syncthreads();
    stamp(0);
    double* cl = base + lay.cl;
    // (side: if the eigenvalues at or below tau come in a cluster of more than TE_SIDE_CL members -- the inverse
    // iteration orthogonalises a cluster in one thread, serially -- the other side is taken after all)
    constexpr int TE_SIDE_CL = 8;
    for (int pass = 0; pass < 2; ++pass) {
        for (int q = t; q < k; q += 256) {  // trisection for the (mt-1-q)-th ascending eigenvalue (side: the q-th)
            const int j = side ? q : mt - 1 - q;
            double lo = gl, hi = gu;
            {   // the first grid point with more than j eigenvalues below it (counts are monotone in x)
                int a0 = 0, a1 = TE_GRID;
                while (a1 - a0 > 1) {
                    const int am = (a0 + a1) >> 1;
                    if (gcnt[am] > j) a1 = am;
                    else a0 = am;
                }
                if (gcnt[a1] > j) {
                    lo = gl + a0 * gh;
                    if (a1 < TE_GRID) hi = gl + a1 * gh;
                }
            }
            for (int it = 0; it < 200; ++it) {
                // LAPACK dstebz's test with its default ABSTOL = ulp ||T||
                if (hi - lo <= fmax(2.0 * eps * fmax(fabs(lo), fabs(hi)), fmax(eps * tn, pivmin))) break;
                const double stp = (hi - lo) * (1.0 / 3.0);
                const double x0 = lo + stp, x1 = fmax(x0, hi - stp);
                int c0, c1;
                sturm_count2(d, e2, mt, x0, x1, pivmin, c0, c1);
                // eigenvalue j lies below x iff more than j eigenvalues do
                if (c0 > j) {
                    hi = x0;
                } else if (c1 > j) {
                    lo = x0;
                    hi = x1;
                } else {
                    lo = x1;
                }
            }
            lam[q] = slam[q] = 0.5 * (lo + hi);
        }
        __syncthreads();
        stamp(1);
        if (t == 0) {
            int nc = 0, mx = 0, cs = 0;   // (cs: the current cluster's first index, in a register)
            double sum = 0.0;
            for (int q = 0; q < k; ++q) {
                if (q == 0 || fabs(slam[q - 1] - slam[q]) >= kOrtol * tn) {
                    cl[nc++] = q;
                    cs = q;
                }
                mx = max(mx, q + 1 - cs);
                sum += slam[q] - tau;
            }
            if (side && mx > TE_SIDE_CL) {   // the eigenvalues above tau instead
                s_side = 0;
                s_k = mt - k;
            } else {
                if (side) {
                    double tr = 0.0;
                    for (int i = 0; i < mt; ++i) tr += d[i];
                    sum = (tr - mt * tau) - sum;
                }
                cl[nc] = k;
                s_ncl = nc;
                base[lay.misc] = k;
                base[lay.misc + 1] = sum;
                base[lay.misc + 2] = side;
                s_side = -1;   // (done)
            }
        }
        __syncthreads();
        if (s_side < 0) break;
        side = s_side;
        k = s_k;
    }
    __syncthreads();
    stamp(2);
    const int ncl = s_ncl;
    double* lu = base + lay.lu;
    double* Z = base + lay.z;
    const double tiny = eps * tn;  // perturb (near-)zero pivots, as dlagts
    for (int c = t; c < ncl; c += 256) {
        const int ln = c % lay.lanes;
        auto at = [&](int arr, int i) -> double& { return lu[((long long)arr * mt + i) * lay.lanes + ln]; };
        const int q0 = (int)cl[c], q1 = (int)cl[c + 1];
        if (q1 - q0 == 1 && twisted_vector(d, e, mt, lam[q0], tiny, Z + (long long)q0 * mt, at)) continue;
        if (q1 - q0 <= TE_TW_CL && twisted_cluster(d, e, mt, slam, q0, q1, tn, tiny, Z, at)) continue;
        for (int q = q0; q < q1; ++q) {
            const double lq = lam[q];
            // dgttrf on T - lq I with the running diagonal / superdiagonal entries carried in
            // registers (every entry is final once its row is passed; the near-zero pivot guard of
            // dlagts is applied as the diagonal entry is stored)
            double cur_d = d[0] - lq, cur_du = e[0];
            for (int i = 0; i + 1 < mt; ++i) {
                const double dli = e[i], nd = d[i + 1] - lq, ndu = e[i + 1];
                double f = dli, u1 = cur_d, u2 = cur_du, u3 = 0.0, piv = 0.0;
                if (fabs(cur_d) >= fabs(dli)) {
                    if (cur_d != 0.0) {
                        f = dli / cur_d;
                        cur_d = nd - f * cur_du;
                    } else {
                        cur_d = nd;
                    }
                    cur_du = ndu;
                } else {
                    f = cur_d / dli;
                    u1 = dli;
                    u2 = nd;
                    cur_d = cur_du - f * nd;
                    if (i + 2 < mt) {
                        u3 = ndu;
                        cur_du = -f * ndu;
                    } else {
                        cur_du = ndu;
                    }
                    piv = 1.0;
                }
                at(0, i) = f;
                at(1, i) = fabs(u1) < tiny ? (u1 < 0.0 ? -tiny : tiny) : u1;
                at(2, i) = u2;
                at(3, i) = u3;
                at(4, i) = piv;
            }
            at(1, mt - 1) = fabs(cur_d) < tiny ? (cur_d < 0.0 ? -tiny : tiny) : cur_d;
            at(2, mt - 1) = cur_du;
            at(3, mt - 1) = 0.0;
            at(4, mt - 1) = 0.0;
            // start vector.  1 + 0.01 sin(.) spans only {1, sin, cos} across q: where T splits and the eigenvalue
            // is exactly multiple, a solve scales the cluster's rows alike, so a fourth member's start lies in the
            // span of the first three, the projection leaves rounding noise, and what the second solve amplifies
            // is noise against the neighbouring eigenvectors' 1 / gap^2 (measured: 8e-11 of a neighbour in the
            // 16th vector of a 16-fold diagonal entry, d = 256).  From the fourth member on the start is a hash of
            // (i, q - q0), uniform in [-1, 1) as LAPACK dstein's dlarnv start; the first three keep their values.
            if (q - q0 < 3) {
                for (int i = 0; i < mt; ++i) at(5, i) = 1.0 + 0.01 * sin(1.0 + 0.7 * i + 1.3 * q);
            } else {
                for (int i = 0; i < mt; ++i) {
                    unsigned h = (unsigned)i * 2654435761u ^ (unsigned)(q - q0) * 0x9E3779B9u;
                    h ^= h >> 15;
                    h *= 0x2C1B3C6Du;
                    h ^= h >> 12;
                    h *= 0x297A2D39u;
                    h ^= h >> 15;
                    at(5, i) = (double)h * 4.656612873077393e-10 - 1.0;   // h 2^-31 - 1
                }
            }
            double* zq = Z + (long long)q * mt;
            // The solves below walk the lane's LU arrays (lane-interleaved global scratch) one row after the
            // other; the loads of a block of TE_PF rows are issued together ahead of the block's dependent
            // chain (they depend on the row index only), so the chain waits for one memory round trip per
            // block instead of one per row.  Same operations in the same order as the row-by-row form.
            // the normalisation of a solve's result is applied as the next solve loads it (sc): the same
            // products fl(y inv) as a separate scaling pass, without its round trips
            double sc = 1.0;
            for (int sweep = 0; sweep < TE_SWEEPS; ++sweep) {
                double cur = at(5, 0) * sc;
                for (int i0 = 0; i0 + 1 < mt; i0 += TE_PF) {  // dgttrs, L
                    double nx[TE_PF], fv[TE_PF], pv[TE_PF];
#pragma unroll
                    for (int u = 0; u < TE_PF; ++u) {
                        const int i = min(i0 + u, mt - 2);
                        nx[u] = at(5, i + 1) * sc;
                        fv[u] = at(0, i);
                        pv[u] = at(4, i);
                    }
#pragma unroll
                    for (int u = 0; u < TE_PF; ++u) {
                        const int i = i0 + u;
                        if (i + 1 >= mt) break;
                        if (pv[u] == 0.0) {
                            at(5, i) = cur;
                            cur = nx[u] - fv[u] * cur;
                        } else {
                            at(5, i) = nx[u];
                            cur = cur - fv[u] * nx[u];
                        }
                    }
                }
                // U back substitution, y_{i+1} and y_{i+2} carried in registers
                double y2 = cur / at(1, mt - 1), y1 = y2;
                double nrm = y2 * y2;
                at(5, mt - 1) = y2;
                if (mt > 1) {
                    y1 = (at(5, mt - 2) - at(2, mt - 2) * y2) / at(1, mt - 2);
                    at(5, mt - 2) = y1;
                    nrm += y1 * y1;
                }
                for (int i0 = mt - 3; i0 >= 0; i0 -= TE_PF) {
                    double yv[TE_PF], u1v[TE_PF], u2v[TE_PF], u3v[TE_PF];
#pragma unroll
                    for (int u = 0; u < TE_PF; ++u) {
                        const int i = max(i0 - u, 0);
                        yv[u] = at(5, i);
                        u1v[u] = at(1, i);
                        u2v[u] = at(2, i);
                        u3v[u] = at(3, i);
                    }
#pragma unroll
                    for (int u = 0; u < TE_PF; ++u) {
                        const int i = i0 - u;
                        if (i < 0) break;
                        const double y = (yv[u] - u2v[u] * y1 - u3v[u] * y2) / u1v[u];
                        at(5, i) = y;
                        nrm += y * y;
                        y2 = y1;
                        y1 = y;
                    }
                }
                if (q > q0) {   // project out the cluster's earlier vectors
                    for (int p = q0; p < q; ++p) {
                        const double* zp = Z + (long long)p * mt;
                        double sp = 0.0;
                        for (int i = 0; i < mt; ++i) sp += zp[i] * at(5, i);
                        for (int i = 0; i < mt; ++i) at(5, i) -= sp * zp[i];
                    }
                    nrm = 0.0;
                    for (int i = 0; i < mt; ++i) nrm += at(5, i) * at(5, i);
                }
                const double inv = 1.0 / sqrt(nrm);
                if (sweep < TE_SWEEPS - 1) {
                    sc = inv;
                } else {   // the vector out, 32 rows per round trip
                    constexpr int TE_CP = 32;
                    for (int i0 = 0; i0 < mt; i0 += TE_CP) {
                        double tv[TE_CP];
#pragma unroll
                        for (int u = 0; u < TE_CP; ++u) tv[u] = at(5, min(i0 + u, mt - 1));
#pragma unroll
                        for (int u = 0; u < TE_CP; ++u)
                            if (i0 + u < mt) zq[i0 + u] = tv[u] * inv;
                    }
                }
            }
        }
    }
    if (t == 0 && status && !(tn >= 0.0)) atomicOr(&status[status_off + b], (int)ACE_ST_EIG_NOCONV);
#ifdef ACE_H2_STAMPS
    stamp(3);
    if (t == 0 && (b % 101) == 0)
        printf("trieig b %d k %d ncl %d: grid %llu bisect %llu clus %llu invit %llu (x10ns)\n", b, k, ncl, st_ph[0],
               st_ph[1], st_ph[2], st_ph[3]);
    __syncthreads();
    if (t == 0) {   // slow work-groups: wall time and the largest cluster
        const unsigned long long wall = __builtin_amdgcn_s_memrealtime() - st_t0;
        if (wall > 180000) {
            int mx = 0;
            for (int c = 0; c < ncl; ++c) mx = max(mx, (int)cl[c + 1] - (int)cl[c]);
            printf("trieig-slow b %d k %d ncl %d maxcl %d wall %llu bisect %llu\n", b, k, ncl, mx, wall, st_ph[1]);
        }
    }
#endif
}

// u_k = H_0 H_1 ... H_{mt-2} z_k  (Q of zhetrd applied to the tridiagonal eigenvectors),
// W_k = D u_k.  Vectors are processed in chunks held in LDS (the in-place updates of a
// vector in global memory would put an L2 store->load round trip between consecutive
// reflectors); within a chunk a 16-lane group owns one vector: segment dot products, a
// 16-lane shuffle reduction and the update, with no barrier per reflector.
constexpr int BX_SEG = 16;                 // lanes per vector
constexpr int BX_REG = 16;                 // register-prefetched elements per lane (mt <= 256)

__device__ __forceinline__ double seg_sum(double v) {  // sum over the 16-lane group
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void backxf_kernel(int mt, int ldw, const double* scratch, SpecLayout lay,
                                                     double* Wout, int scale_d, const int* active, int cv) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (active && !active[b]) return;
    extern __shared__ double smem[];
    d2* U = reinterpret_cast<d2*>(smem);   // [cv][mt]
    const double* base = scratch + b * lay.stride;
    const int r = (int)base[lay.misc];
    const d2* C = reinterpret_cast<const d2*>(base + lay.C);
    const d2* taus = reinterpret_cast<const d2*>(base + lay.tau);
    const double* dv = base + lay.dv;
    d2* W = reinterpret_cast<d2*>(Wout) + (long long)b * ldw * mt;
    const int grp = t / BX_SEG, sl = t % BX_SEG;
    const bool owner = grp < cv;
    for (int k0 = 0; k0 < r; k0 += cv) {
        const int k = k0 + grp;
        const bool mine = owner && k < r;
        d2* u = U + (long long)grp * mt;
        if (mine) {
            const double* z = base + lay.z + (long long)k * mt;
            for (int i = sl; i < mt; i += BX_SEG) u[i] = make_double2(z[i], 0.0);
        }
        // reflectors j = mt-2 .. 0 act on u[j+1 ..]; v_j[0] = 1 sits at C[j][j+1]
        if (mine && mt <= BX_SEG * BX_REG) {  // reflector segments double-buffered in registers
            d2 vc[BX_REG], vn[BX_REG];
            auto fetch = [&](int j, d2 (&dst)[BX_REG]) {
                const int L = mt - j - 1;
                const d2* v = C + (long long)j * mt + j + 1;
#pragma unroll
                for (int p = 0; p < BX_REG; ++p) {
                    const int i = sl + BX_SEG * p;
                    dst[p] = i < L ? v[i] : make_double2(0.0, 0.0);
                }
            };
            fetch(mt - 2, vn);
            for (int j = mt - 2; j >= 0; --j) {
#pragma unroll
                for (int p = 0; p < BX_REG; ++p) vc[p] = vn[p];
                if (j > 0) fetch(j - 1, vn);
                const d2 tau = taus[j];
                if (tau.x == 0.0 && tau.y == 0.0) continue;
                const int L = mt - j - 1;
                d2* uj = u + j + 1;
                double sr = 0.0, si = 0.0;
#pragma unroll
                for (int p = 0; p < BX_REG; ++p) {
                    const int i = sl + BX_SEG * p;
                    if (i < L) {
                        const d2 q = cmulc(vc[p], uj[i]);
                        sr += q.x;
                        si += q.y;
                    }
                }
                sr = seg_sum(sr);
                si = seg_sum(si);
                const d2 f = cmul(tau, make_double2(sr, si));
#pragma unroll
                for (int p = 0; p < BX_REG; ++p) {
                    const int i = sl + BX_SEG * p;
                    if (i < L) uj[i] = csub(uj[i], cmul(f, vc[p]));
                }
            }
        } else if (mine) {
            for (int j = mt - 2; j >= 0; --j) {
                const d2 tau = taus[j];
                if (tau.x == 0.0 && tau.y == 0.0) continue;
                const int L = mt - j - 1;
                const d2* v = C + (long long)j * mt + j + 1;
                d2* uj = u + j + 1;
                double sr = 0.0, si = 0.0;
                for (int i = sl; i < L; i += BX_SEG) {
                    const d2 q = cmulc(v[i], uj[i]);
                    sr += q.x;
                    si += q.y;
                }
                sr = seg_sum(sr);
                si = seg_sum(si);
                const d2 f = cmul(tau, make_double2(sr, si));
                for (int i = sl; i < L; i += BX_SEG) uj[i] = csub(uj[i], cmul(f, v[i]));
            }
        }
        if (mine) {
            d2* w = W + (long long)k * mt;
            for (int i = sl; i < mt; i += BX_SEG) w[i] = scale_d ? cscale(u[i], dv[i]) : u[i];
        }
    }
}
// vectors per back-transform chunk: 16 (one per 16-lane group) within 64 KiB of LDS
int backxf_chunk(int mt) {
    int cv = (64 * 1024) / (16 * mt);
    return cv < 1 ? 1 : (cv > 16 ? 16 : cv);
}
}  // namespace
// dynamic LDS of hetrd_kernel / hetrd_blk_kernel at order d (ace_lds_request)
size_t hetrd_request_bytes(int d, int blk) {   // (blk: the larger of the prox's and the spectral panel widths)
    return blk ? std::max(hetrd_blk_lds(d, HB_NB), hetrd_blk_lds(d, HB_NB_SPEC)) : hetrd_lds(d);
}

namespace {
// ---- primal form for m_t > n: the n x n Gram As^H As itself (a smaller eigenproblem)
// Ast[b][i][k] = w_b[k] A_t^H[i][k], w_b[k] = B_t[b][k]^2 / ||a_k||^2 (0 for a zero row), so that
// one batched GEMM C_b = conj(Ast_b) applied to the rows of A_t^H gives As^H As row by row.
// mask (PartRows): mt is then the full m, A_t^H the full A^H and B_t the full B row; the weight of a test
// row is zero, so the GEMM below sums the realisation's own train rows (in ascending row order)
__global__ __launch_bounds__(256) void spec_weight_kernel(int mt, int n, int nb, const double* Kp, const double* AHp,
                                                          const double* Bt, double* Astp, const unsigned char* mask,
                                                          int ldmask) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)n * mt;
    if (e >= per * nb) return;
    const int b = (int)(e / per), k = (int)(e % mt);
    const double kkk = reinterpret_cast<const d2*>(Kp)[(long long)k * mt + k].x;
    const double bk = Bt[(long long)b * mt + k];
    const double wk = (kkk > 0.0 && !(mask && !mask[(long long)b * ldmask + k])) ? bk * bk / kkk : 0.0;
    const d2 a = reinterpret_cast<const d2*>(AHp)[e % per];
    reinterpret_cast<d2*>(Astp)[e] = make_double2(wk * a.x, wk * a.y);
}
// C_b <- (C_b + C_b^H) / 2 in place (the oracle's symmetrisation), one thread per pair i <= j
__global__ __launch_bounds__(256) void spec_herm_kernel(int n, double* scratch, SpecLayout lay) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 16 + threadIdx.x / 16, j = (int)(threadIdx.x % 16) + blockIdx.z * 16;
    if (i >= n || j >= n || j < i) return;
    d2* C = reinterpret_cast<d2*>(scratch + b * lay.stride + lay.C);
    const d2 a = C[(long long)i * n + j], c = C[(long long)j * n + i];
    const d2 h = make_double2(0.5 * (a.x + c.x), 0.5 * (a.y - c.y));
    C[(long long)i * n + j] = i == j ? make_double2(h.x, 0.0) : h;
    if (i != j) C[(long long)j * n + i] = make_double2(h.x, -h.y);
}
// X[b][k][:] *= sqrt(max(0, lam_k))  (SpectralInitialize :571-573)
__global__ __launch_bounds__(256) void spec_sqrt_scale_kernel(int n, int r, const double* scratch, SpecLayout lay,
                                                              double* Xp) {
    const int b = blockIdx.y, k = blockIdx.x;
    const double lam = scratch[b * lay.stride + lay.lam + k];
    const double s = sqrt(lam > 0.0 ? lam : 0.0);
    d2* x = reinterpret_cast<d2*>(Xp) + ((long long)b * r + k) * n;
    for (int i = threadIdx.x; i < n; i += 256) x[i] = cscale(x[i], s);
}
constexpr size_t PRIMAL_AST_BYTES = 256ull << 20;   // weighted A_t^H images per chunk
int primal_chunk(int mt, int n, int batch) {
    long long c = (long long)(PRIMAL_AST_BYTES / (16ull * n * mt));
    if (c < 1) c = 1;
    if (c > SPEC_CHUNK) c = SPEC_CHUNK;
    return (int)(c < batch ? c : batch);
}
}  // namespace

bool spectral_primal(int mt, int n) { return mt > n; }

size_t spectral_scratch_bytes(int mt, int n, int batch, int r) {
    if (spectral_primal(mt, n)) {
        const SpecLayout lay(n, r);
        const int chunk = primal_chunk(mt, n, batch);
        return (sizeof(double) * (size_t)lay.stride + 16ull * n * mt + 256) * chunk;
    }
    const SpecLayout lay(mt, r);
    const int chunk = batch < SPEC_CHUNK ? batch : SPEC_CHUNK;
    return sizeof(double) * (size_t)lay.stride * chunk;
}

// the spectral initialisation's tridiagonalisation: the panel-blocked reduction when its LDS fits (order
// <= ~560); ACE_HETRD_BLK=0 keeps hetrd_kernel (A/B; read once per process)
static bool spectral_blk() {
    static const bool v = [] {
        const char* e = getenv("ACE_HETRD_BLK");
        return !(e && e[0] == '0');
    }();
    return v;
}

int launch_spectral_primal(int mt, int n, int r, int batch, const double* K, const double* AH, const double* Bt,
                           double* scratch, double* X, int* status, hipStream_t st, const PartRows* pr) {
    if (pr) mt = pr->m;   // the full A^H, B and K; test rows weighted zero
    const SpecLayout lay(n, r);
    const size_t sm_h = hetrd_lds(n), sm_t = trieig_lds(n);
    if (!hetrd_lds_ok(n)) return ACE_ERR_UNSUPPORTED;
    const bool blk = spectral_blk() &&
                     lds_ok(reinterpret_cast<const void*>(&hetrd_blk_kernel<HB_NB_SPEC>), hetrd_blk_lds(n, HB_NB_SPEC));
    const int chunk = primal_chunk(mt, n, batch);
    double* Ast = scratch + (((size_t)lay.stride * chunk + 31) & ~(size_t)31);
    for (int b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = batch - b0 < chunk ? batch - b0 : chunk;
        const long long elems = (long long)nb * n * mt;
        hipLaunchKernelGGL(spec_weight_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, mt, n, nb, K, AH,
                           Bt + (long long)b0 * mt, Ast, pr ? pr->mask + (long long)b0 * pr->ldmask : nullptr,
                           pr ? pr->ldmask : 0);
        // C_b[v][i] = sum_k w_k A_t[k][i] conj(A_t[k][v]) = (As^H As)[v][i]
        launch_zgemm(0, true, n, mt, n, Ast, mt, (long long)n * mt, AH, mt, 0, scratch + lay.C, nullptr, n,
                     lay.stride / 2, nb, st);
        hipLaunchKernelGGL(spec_herm_kernel, dim3((n + 15) / 16, nb, (n + 15) / 16), dim3(256), 0, st, n, scratch, lay);
        if (blk)
            hipLaunchKernelGGL(hetrd_blk_kernel<HB_NB_SPEC>, dim3(nb), dim3(HB_THREADS), hetrd_blk_lds(n, HB_NB_SPEC), st, n,
                               scratch, lay, nullptr);
        else
            hipLaunchKernelGGL(hetrd_kernel, dim3(nb), dim3(HT_THREADS), sm_h, st, n, nullptr, nullptr, scratch, lay,
                               nullptr, nullptr, 0);
        hipLaunchKernelGGL(trieig_kernel, dim3(nb), dim3(256), sm_t, st, n, nullptr, scratch, lay, status, b0, nullptr, 0);
        const int cv = backxf_chunk(n);
        double* Xb = X + 2LL * b0 * r * n;
        hipLaunchKernelGGL(backxf_kernel, dim3(nb), dim3(256), (size_t)cv * n * 16, st, n, r, scratch, lay, Xb, 0,
                           nullptr, cv);
        hipLaunchKernelGGL(spec_sqrt_scale_kernel, dim3(r, nb), dim3(256), 0, st, n, r, scratch, lay, Xb);
    }
    return ACE_OK;
}

int launch_spectral(int mt, int r, int batch, const double* K, const double* Bt, double* scratch, double* W,
                    int* status, hipStream_t st, const PartRows* pr) {
    const SpecLayout lay(mt, r);
    const size_t sm_h = hetrd_lds(mt), sm_t = trieig_lds(mt);
    if (!hetrd_lds_ok(mt)) return ACE_ERR_UNSUPPORTED;
    const bool blk = spectral_blk() &&
                     lds_ok(reinterpret_cast<const void*>(&hetrd_blk_kernel<HB_NB_SPEC>), hetrd_blk_lds(mt, HB_NB_SPEC));
    const int ldb = pr ? pr->m : mt;   // per-realisation partitions: the full K and B, rows per realisation
    for (int b0 = 0; b0 < batch; b0 += SPEC_CHUNK) {
        const int nb = batch - b0 < SPEC_CHUNK ? batch - b0 : SPEC_CHUNK;
        if (blk) {   // C formed first, then the panel-blocked reduction (r05)
            hipLaunchKernelGGL(spec_form_c_kernel, dim3(nb), dim3(256), (size_t)mt * sizeof(double), st, mt, K,
                               Bt + (long long)b0 * ldb, scratch, lay, pr ? pr->rows + (long long)b0 * pr->m : nullptr,
                               pr ? pr->m : 0);
            hipLaunchKernelGGL(hetrd_blk_kernel<HB_NB_SPEC>, dim3(nb), dim3(HB_THREADS), hetrd_blk_lds(mt, HB_NB_SPEC), st, mt,
                               scratch, lay, nullptr);
        } else {
            hipLaunchKernelGGL(hetrd_kernel, dim3(nb), dim3(HT_THREADS), sm_h, st, mt, K, Bt + (long long)b0 * ldb, scratch,
                               lay, nullptr, pr ? pr->rows + (long long)b0 * pr->m : nullptr, pr ? pr->m : 0);
        }
        hipLaunchKernelGGL(trieig_kernel, dim3(nb), dim3(256), sm_t, st, mt, nullptr, scratch, lay, status, b0, nullptr, 0);
        const int cv = backxf_chunk(mt);
        hipLaunchKernelGGL(backxf_kernel, dim3(nb), dim3(256), (size_t)cv * mt * 16, st, mt, r, scratch, lay,
                           W + 2LL * b0 * r * mt, 1, nullptr, cv);
    }
    return ACE_OK;
}

// ---- blocked (compact-WY) back-transform for many eigenvectors (PhaseLift's prox_trace keeps
// 100-256 of d = 256).  zhetrd's Q = H_0 H_1 ... H_{d-2}; per block of WY_NB consecutive
// reflectors Q_j = I - V_j T_j V_j^H (LAPACK zlarft, forward, columnwise), and
// Q z = Q_0 (Q_1 ( ... Q_last z)) is three batched MFMA GEMMs per block over all vectors:
//   W1 = V_j^H Z,  W2 = T_j W1,  Z -= V_j W2.
// V_j^H reads the reflectors where hetrd left them (row k of C, C[k][k+1] = 1; the stale entries
// left of it are zeroed by wy_pack_kernel), V_j comes from a transposed copy (VT_j), and the
// Gram V_j^H V_j that zlarft needs is one more GEMM.
namespace {
constexpr int WY_NB = 64;
struct WyLayout {            // per realisation, in doubles
    long long VT, Tm, Gm, W1, W2, stride;
    int nblk;
    WyLayout(int d, int kmax) {
        nblk = (d - 1 + WY_NB - 1) / WY_NB;
        long long o = 0;
        auto take = [&](long long nd) { long long p = o; o += (nd + 31) & ~31LL; return p; };
        VT = take(2LL * nblk * d * WY_NB);     // block j: [L_j][WY_NB] at VT + 2 j d WY_NB
        Tm = take(2LL * nblk * WY_NB * WY_NB);
        Gm = take(2LL * nblk * WY_NB * WY_NB);
        W1 = take(2LL * kmax * WY_NB);
        W2 = take(2LL * kmax * WY_NB);
        stride = o;
    }
};
bool wy_path(int d, int kmax) { return d >= 96 && kmax >= 32; }

// zero what is not reflector in rows 0..d-2 of C (left of C[k][k+1] within the row's block, and the
// whole row when tau_k = 0: H_k = I) and write VT_j[p][a] = v_{j0+a}[j0+1+p]
__global__ __launch_bounds__(256) void wy_pack_kernel(int d, double* scratch, SpecLayout lay, double* wy, WyLayout wl,
                                                      const int* active) {
    const int b = blockIdx.x;
    if (active && !active[b]) return;
    double* base = scratch + b * lay.stride;
    d2* C = reinterpret_cast<d2*>(base + lay.C);
    const d2* taus = reinterpret_cast<const d2*>(base + lay.tau);
    d2* VT = reinterpret_cast<d2*>(wy + b * wl.stride + wl.VT);
    for (int j = 0; j < wl.nblk; ++j) {
        const int j0 = j * WY_NB, L = d - j0 - 1;
        d2* vt = VT + (long long)j * d * WY_NB;
        for (long long e = threadIdx.x; e < (long long)L * WY_NB; e += 256) {
            const int p = (int)(e / WY_NB), a = (int)(e % WY_NB), k = j0 + a;
            d2 v = make_double2(0.0, 0.0);
            if (k < d - 1) {
                const d2 tk = taus[k];
                d2& c = C[(long long)k * d + j0 + 1 + p];
                if (p < a || (tk.x == 0.0 && tk.y == 0.0)) c = make_double2(0.0, 0.0);
                else v = c;
            }
            vt[e] = v;
        }
    }
}

// T_j (upper triangular, row-major [a][c]) from the Gram G[v][i] = (V^H V)[i][v] (zlarft):
// T[i][i] = tau_i,  T[0:i][i] = -tau_i T[0:i][0:i] (V^H V)[0:i][i]
__global__ __launch_bounds__(64) void wy_larft_kernel(int d, const double* scratch, SpecLayout lay, double* wy,
                                                      WyLayout wl, const int* active) {
    const int j = blockIdx.x, b = blockIdx.y, a = threadIdx.x;
    if (active && !active[b]) return;
    __shared__ d2 T[WY_NB][WY_NB + 1];
    __shared__ d2 y[WY_NB];
    const d2* taus = reinterpret_cast<const d2*>(scratch + b * lay.stride + lay.tau);
    const d2* G = reinterpret_cast<const d2*>(wy + b * wl.stride + wl.Gm) + (long long)j * WY_NB * WY_NB;
    d2* Tg = reinterpret_cast<d2*>(wy + b * wl.stride + wl.Tm) + (long long)j * WY_NB * WY_NB;
    const int j0 = j * WY_NB, nbj = min(WY_NB, d - 1 - j0);
    for (int c = 0; c < WY_NB; ++c) T[a][c] = make_double2(0.0, 0.0);
    // step i's G row and tau are loaded during step i - 1 (the loads do not depend on the recurrence)
    d2 gn = G[a], tn = taus[j0];
    __syncthreads();
    for (int i = 0; i < nbj; ++i) {
        const d2 ti = tn, gi = gn;
        if (i + 1 < nbj) {
            gn = G[(long long)(i + 1) * WY_NB + a];
            tn = taus[j0 + i + 1];
        }
        if (a < i) y[a] = cscale(cmul(ti, gi), -1.0);
        __syncthreads();
        if (a < i) {
            d2 acc = make_double2(0.0, 0.0);
            for (int c = a; c < i; ++c) acc = cadd(acc, cmul(T[a][c], y[c]));
            T[a][i] = acc;
        }
        if (a == 0) T[i][i] = ti;
        __syncthreads();
    }
    for (int c = 0; c < WY_NB; ++c) Tg[(long long)a * WY_NB + c] = T[a][c];
}

// V[b][q][:] = z_q (real tridiagonal eigenvector) for q < k_b, 0 for k_b <= q < kuse
__global__ __launch_bounds__(256) void wy_expand_kernel(int d, int kuse, const double* scratch, SpecLayout lay,
                                                        double* Vout, int ldv, const int* active) {
    const int b = blockIdx.y;
    if (active && !active[b]) return;
    const double* base = scratch + b * lay.stride;
    const int k = (int)base[lay.misc];
    d2* V = reinterpret_cast<d2*>(Vout) + (long long)b * ldv * d;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < (long long)kuse * d; e += 256LL * gridDim.x) {
        const int q = (int)(e / d);
        V[e] = make_double2(q < k ? base[lay.z + e] : 0.0, 0.0);
    }
}

// kmax_out[0] = max over active realisations of k_b
__global__ __launch_bounds__(256) void wy_kmax_kernel(int batch, const double* scratch, SpecLayout lay,
                                                      const int* active, int* kmax_out) {
    int k = 0;
    for (int b = threadIdx.x; b < batch; b += 256)
        if (!active || active[b]) k = max(k, (int)scratch[b * lay.stride + lay.misc]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k = max(k, __shfl_xor(k, o, 64));
    __shared__ int s[4];
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = k;
    __syncthreads();
    if (threadIdx.x == 0) kmax_out[0] = max(max(s[0], s[1]), max(s[2], s[3]));
}
}  // namespace

// ---- thresholded / top-k Hermitian eigen (PhaseLift prox_trace and its final eig): see ace_pipe.hpp
HeevLayout heev_layout(int d, int kmax) {
    const SpecLayout lay(d, kmax);
    return HeevLayout{lay.stride, lay.C, lay.misc, lay.lam, lay.dd, lay.ee, lay.z};
}
size_t heev_scratch_bytes(int d, int kmax, int batch) {
    size_t b = sizeof(double) * (size_t)SpecLayout(d, kmax).stride * batch, x = 0;
    if (wy_path(d, kmax)) x = sizeof(double) * (size_t)WyLayout(d, kmax).stride * batch + 256;
    if (heev2_eligible(d, kmax)) x = std::max(x, heev2_extra_bytes(d, batch));
    return b + x;
}

void launch_trieig(int d, int kmax, int batch, const double* tau, double* scratch, int* status, const int* active,
                   hipStream_t st, int side_ok) {
    const SpecLayout lay(d, kmax);
    hipLaunchKernelGGL(trieig_kernel, dim3(batch), dim3(256), trieig_lds(d), st, d, tau, scratch, lay, status, 0, active,
                       side_ok);
}

int launch_heev(int d, int kmax, int batch, const double* tau, double* scratch, double* V, int* status,
                const int* active, hipStream_t st, int path, int side_ok) {
    side_ok = side_ok && tau && kmax == d;
    if (path == 2 && heev2_eligible(d, kmax))
        return launch_heev2(d, kmax, batch, tau, scratch, V, status, active, st, side_ok);
    int blk = path != 0;
    const SpecLayout lay(d, kmax);
    const size_t sm_h = hetrd_lds(d), sm_t = trieig_lds(d);
    if (!hetrd_lds_ok(d)) return ACE_ERR_UNSUPPORTED;
    // the blocked reduction (hetrd_blk_kernel): blk = 1 (the caller reads ACE_HETRD_BLK once per solve)
    // (a check that records nothing: the unblocked reduction takes any d hetrd_lds_ok admits, so a blocked form
    // that does not fit is a choice of path, not a refused launch)
    if (blk && !lds_ok(reinterpret_cast<const void*>(&hetrd_blk_kernel<HB_NB>), hetrd_blk_lds(d))) blk = 0;
    if (blk) {
        // (all matrices in one launch: launches of 128 / 256 matrices, whose working set would stay in the MALL,
        // measured 37.8 / 54.1 against 60.4 rec/s -- the reduction is bound by its work-groups' latency, not HBM)
        hipLaunchKernelGGL(hetrd_blk_kernel<HB_NB>, dim3(batch), dim3(HB_THREADS), hetrd_blk_lds(d), st, d, scratch, lay, active);
    } else {
        hipLaunchKernelGGL(hetrd_kernel, dim3(batch), dim3(HT_THREADS), sm_h, st, d, nullptr, nullptr, scratch, lay, active,
                           nullptr, 0);
    }
    hipLaunchKernelGGL(trieig_kernel, dim3(batch), dim3(256), sm_t, st, d, tau, scratch, lay, status, 0, active, side_ok);
    if (!wy_path(d, kmax)) {
        const int cv = backxf_chunk(d);
        hipLaunchKernelGGL(backxf_kernel, dim3(batch), dim3(256), (size_t)cv * d * 16, st, d, kmax, scratch, lay, V, 0,
                           active, cv);
        return ACE_OK;
    }
    const WyLayout wl(d, kmax);
    double* wy = scratch + (size_t)lay.stride * batch;
    int* kdev = reinterpret_cast<int*>(wy + (size_t)wl.stride * batch);
    hipLaunchKernelGGL(wy_kmax_kernel, dim3(1), dim3(256), 0, st, batch, scratch, lay, active, kdev);
    int kuse = 0;
    if (read_back(&kuse, kdev, sizeof(int), st) != hipSuccess) return ACE_ERR_HIP;
    if (kuse <= 0) return ACE_OK;   // nothing above the threshold anywhere (callers read k_b = 0)
    if (kuse > kmax) kuse = kmax;
    hipLaunchKernelGGL(wy_pack_kernel, dim3(batch), dim3(256), 0, st, d, scratch, lay, wy, wl, active);
    const long long sC = lay.stride / 2, sW = wl.stride / 2, sV = (long long)kmax * d;
    for (int j = 0; j < wl.nblk; ++j) {   // Gram V_j^H V_j
        const int j0 = j * WY_NB, nbj = std::min(WY_NB, d - 1 - j0), L = d - j0 - 1;
        const double* Vr = scratch + lay.C + 2LL * ((long long)j0 * d + j0 + 1);
        launch_zgemm(0, true, nbj, L, nbj, Vr, d, sC, Vr, d, sC, wy + wl.Gm + 2LL * j * WY_NB * WY_NB, nullptr, WY_NB,
                     sW, batch, st);
    }
    hipLaunchKernelGGL(wy_larft_kernel, dim3(wl.nblk, batch), dim3(64), 0, st, d, scratch, lay, wy, wl, active);
    hipLaunchKernelGGL(wy_expand_kernel, dim3((kuse * d + 255) / 256 < 64 ? (kuse * d + 255) / 256 : 64, batch),
                       dim3(256), 0, st, d, kuse, scratch, lay, V, kmax, active);
    for (int j = wl.nblk - 1; j >= 0; --j) {
        const int j0 = j * WY_NB, nbj = std::min(WY_NB, d - 1 - j0), L = d - j0 - 1;
        const double* Vr = scratch + lay.C + 2LL * ((long long)j0 * d + j0 + 1);
        double* Zj = V + 2LL * (j0 + 1);
        launch_zgemm(0, true, nbj, L, kuse, Vr, d, sC, Zj, d, sV, wy + wl.W1, nullptr, WY_NB, sW, batch, st);
        launch_zgemm(0, false, nbj, nbj, kuse, wy + wl.Tm + 2LL * j * WY_NB * WY_NB, WY_NB, sW, wy + wl.W1, WY_NB, sW,
                     wy + wl.W2, nullptr, WY_NB, sW, batch, st);
        launch_zgemm(1, false, L, nbj, kuse, wy + wl.VT + 2LL * j * d * WY_NB, WY_NB, sW, wy + wl.W2, WY_NB, sW, Zj,
                     Zj, d, sV, batch, st);
    }
    return ACE_OK;
}

}  // namespace ace
