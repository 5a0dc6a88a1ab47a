// Batched orthogonal matching pursuit against one shared dictionary (the sparse stage of the two-stage PLOMP
// recovery, My_TwoStage_Recovery.m, and the OMP branch of My_Conventional_CS.m; OMP.m itself is an external
// toolbox file and is not in the reference tree, so this is textbook OMP with both stopping rules):
//
//   r = y, I = {}
//   repeat: stop if |I| = kmax or ||r||_2 <= tol
//           j = argmax over j not in I of w_j |d_j^H r|^2        (ties: smaller j; w = colscale or 1)
//           I <- I u {j};  c = argmin ||y - D_I c||_2;  r = y - D_I c
//
// One kernel, one launch.  A work-group (8 waves) owns OM_RB = 16 realisations and runs all their iterations
// to the end; a realisation that has stopped idles (its residual row is zeroed, it offers nothing), and the
// work-group leaves when all of its realisations have stopped.  Nothing is combined across work-groups and
// there are no atomics.
//
// Correlation step (the hot part).  D^H R for the block is one complex GEMM, N x d x 16, on
// v_mfma_f64_16x16x4_f64 in the 3M form (mma3m / comb3m of ace_mfma.hpp: three real products per complex
// k-step instead of four; its error is of the order d u sum |d_ej| |r_e| per entry like the 4M form's, which is
// far below what a selection needs, and the values feed nothing but the selection).  The residuals are the B
// operand and stay in LDS (Rs, 16 rows of stride DP + 1, zero-padded to DP = 16 ceil(d / 16)).  D is the A
// operand, conjugated on the way in (a sign flip, exact).  D is row-major [d][N], so the 16 lanes of a
// fragment row read 16 consecutive atoms of one row e, 256 contiguous bytes: the fragments are loaded
// straight from global memory (L2 / Infinity Cache) into registers, no LDS staging, since an entry of D is
// used by exactly one wave of the work-group.  A wave walks pairs of 16-atom tiles (OM_TW = 2, sharing the
// residual reads), in chunks of 4 k-steps with two register sets: the loads of a chunk are issued before the
// MFMAs of the chunk ahead of it.  Rows e >= d and atoms j >= N are masked at the loads (zero fill adds exact
// zeros); nothing is read past the end of D.
// Epilogue: |.|^2 w_j, the exclusion of chosen atoms (a bitmap in LDS) and the running argmax per lane; the
// N-long correlation vector never goes to memory.  The argmax uses the strict total order "value larger, or
// equal and index smaller" (as the scan's top-K), so the winner does not depend on which lane, wave or
// sequence met the candidates: lanes fold over their atoms, the wave folds by two xor shuffles, the eight
// waves' candidates are folded by the realisation's group.
//
// Least-squares step: progressive QR of D_I by modified Gram-Schmidt.  A group of 32 lanes owns a realisation
// (entry e on lane e & 31).  The new atom is orthogonalised against q_0 .. q_{k-1} in sequence
// (rho_i = q_i^H v, v -= rho_i q_i), normalised to q_k, and the residual is updated by
// z_k = q_k^H r, r -= z_k q_k: d MACs, and r never has to be rebuilt from y.  Q [kmax][d], the upper factor
// (column k: rho_0 .. rho_{k-1}, ||v||) and z live in the caller's workspace (2 MB per realisation at
// d = kmax = 256: they do not fit LDS); every entry is written and later read by the same thread.  The
// coefficients follow once, when the realisation stops, by back substitution R c = z.  QR rather than a
// Cholesky factor of the Gram matrix: the coefficients' error grows with kappa_2(D_I), not its square.
//
// Dependence.  If the orthogonalised atom has ||v|| <= 2^-26 ||d_j|| (sqrt(u)), the atom is not added: with
// it kappa_2(D_I) >= 2^26, the direction of v would carry fewer than half its digits (its rounding error
// is of the order k u ||d_j||), and so would the coefficients.  The realisation stops with
// ACE_ST_OMP_DEPENDENT.  An all-zero atom is dependent by the same test.
//
// Batch invariance.  A realisation's outputs are a function of (y_b, D, colscale, d, N, kmax, tol) alone: its
// column of the MFMA results does not depend on the other columns, the tile walk depends on N only, all sums
// have a fixed order, and the selection is order-free.
//
// LDS: 16 (DP + 1) complex for the residuals + 16 x 513 words of bitmap (sized for N = 16384 at every shape)
// = 98624 B at d = 256, dynamic, through the kernel's derived budget (lds_dyn_budget; no second path), plus
// 1792 B static for the waves' candidates.  236 VGPRs, no spill: one work-group per CU, two waves per SIMD.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

namespace ace {
namespace {

constexpr int OM_WAVES = 8;
constexpr int OM_NT = 64 * OM_WAVES;
constexpr int OM_RB = 16;              // realisations per work-group (the columns of one MFMA tile)
constexpr int OM_GL = OM_NT / OM_RB;   // lanes of a realisation's group
constexpr int OM_DMAX = 256;           // largest d
constexpr int OM_NMAX = 16384;         // largest N
constexpr int OM_NU = OM_DMAX / OM_GL; // entries of a d-vector per lane of the group
constexpr int OM_TW = 2;               // atom tiles per wave and pass
constexpr int OM_SK = 4;               // k-steps per chunk
constexpr int OM_BMW = OM_NMAX / 32 + 1;   // bitmap row stride (words; odd: the 16 rows fall on distinct banks)
constexpr double OM_DEP = 0x1p-26;     // dependence threshold on ||v|| / ||d_j||
static_assert(OM_GL == 32 && OM_NU * OM_GL == OM_DMAX, "group layout");

__device__ __forceinline__ bool om_before(double P, int f, double Q, int g) { return P > Q || (P == Q && f < g); }

// sum over the 32 lanes of a group (rows 2h, 2h + 1 of the wave): the same value, bit for bit, in all of them
__device__ __forceinline__ double om_gsum(double v) { return xor16_sum(bsum16(v)); }

constexpr size_t om_lds_bytes(int d) {
    return (size_t)OM_RB * ((d + 15) / 16 * 16 + 1) * sizeof(d2) + (size_t)OM_RB * OM_BMW * sizeof(uint32_t);
}
// workspace per realisation (complex entries): Q [kmax][d], the upper factor [kmax][kmax], z [kmax]
constexpr size_t om_ws_entries(int d, int kmax) { return (size_t)kmax * d + (size_t)kmax * kmax + (size_t)kmax; }

__global__ __launch_bounds__(OM_NT) void omp_kernel(int batch, int d, int N, int kmax, double tol,
                                                    const d2* __restrict__ D, const double* __restrict__ colscale,
                                                    const d2* __restrict__ Y, int32_t* __restrict__ idx,
                                                    d2* __restrict__ coef, int32_t* __restrict__ count,
                                                    double* __restrict__ resnorm, uint32_t* __restrict__ status,
                                                    d2* __restrict__ xout, d2* __restrict__ ws) {
    extern __shared__ __align__(16) unsigned char om_lds[];   // Rs[16][DP + 1], bm[16][OM_BMW] (om_lds_bytes)
    const int DP = (d + 15) / 16 * 16, ST = DP + 1;
    d2* const Rs = (d2*)om_lds;
    uint32_t* const bm = (uint32_t*)(Rs + OM_RB * ST);
    __shared__ double wbv[OM_WAVES][OM_RB];
    __shared__ int wbj[OM_WAVES][OM_RB];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int g = t / OM_GL, gl = t % OM_GL;          // the group's realisation column and the lane within it
    const long long b = (long long)blockIdx.x * OM_RB + g;
    const bool live = b < batch;
    const int nu = (d + OM_GL - 1) / OM_GL;
    const int nst = DP / (4 * OM_SK);                 // chunks of the k loop
    const int ntile = (N + 15) / 16, npair = (ntile + OM_TW - 1) / OM_TW;

    // workspace of the realisation
    d2* const Qb = ws + (live ? (size_t)b : 0) * om_ws_entries(d, kmax);
    d2* const Fb = Qb + (size_t)kmax * d;             // factor, column k at Fb + k kmax
    d2* const zb = Fb + (size_t)kmax * kmax;

    // ---------------- start: r = y, the bitmap cleared, ||y||
    for (int i = t; i < OM_RB * OM_BMW; i += OM_NT) bm[i] = 0u;
    for (int e = gl; e < ST; e += OM_GL) Rs[g * ST + e] = make_double2(0.0, 0.0);
    int mine = 0;
    double s2 = 0.0;
    if (live)
        for (int u = 0; u < nu; ++u) {
            const int e = gl + OM_GL * u;
            if (e < d) {
                const d2 v = Y[(size_t)b * d + e];
                mine |= !isfinite(v.x) || !isfinite(v.y);
                s2 += cabs2(v);
                Rs[g * ST + e] = v;
            }
        }
    const bool bad = ((__ballot(mine) >> (lane & 32)) & 0xffffffffull) != 0ull;   // over the group's half of the wave
    double rn = bad ? 0.0 : sqrt(om_gsum(s2));
    int k = 0;
    uint32_t stat = bad ? ACE_ST_EVAL_DEGENERATE : 0u;
    bool active = live && !bad && rn > tol;
    if (!active)   // an idle realisation's residual row is zero: it adds exact zeros to the products
        for (int e = gl; e < DP; e += OM_GL) Rs[g * ST + e] = make_double2(0.0, 0.0);

    const int frow = (lane & 15) * ST + (lane >> 4);   // residual fragment: row l & 15, k = 4 kk + (l >> 4)

    while (true) {
        if (__syncthreads_or(active) == 0) break;   // (also: Rs and bm of the last step are in place)

        // ================= correlation: wave w walks the tile pairs w, w + 8, ...
        double bv = -1.0;
        int bj = -1;
        for (int tp = w; tp < npair; tp += OM_WAVES) {
            const int j0 = tp * (16 * OM_TW);
            d2 fa[OM_TW][OM_SK], fb[OM_TW][OM_SK];
            d4v p1[OM_TW], p2[OM_TW], p3[OM_TW];
#pragma unroll
            for (int c = 0; c < OM_TW; ++c) p1[c] = p2[c] = p3[c] = d4v{0.0, 0.0, 0.0, 0.0};
            auto gload = [&](d2(&f)[OM_TW][OM_SK], int s) {
#pragma unroll
                for (int kk = 0; kk < OM_SK; ++kk) {
                    const int e = 4 * (OM_SK * s + kk) + (lane >> 4);
#pragma unroll
                    for (int c = 0; c < OM_TW; ++c) {
                        const int j = j0 + 16 * c + (lane & 15);
                        f[c][kk] = make_double2(0.0, 0.0);
                        if (e < d && j < N) f[c][kk] = D[(size_t)e * N + j];
                    }
                }
            };
            auto comp = [&](const d2(&f)[OM_TW][OM_SK], int s) {
#pragma unroll
                for (int kk = 0; kk < OM_SK; ++kk) {
                    const d2 r = Rs[frow + 4 * (OM_SK * s + kk)];
                    const double rs = r.x + r.y;
#pragma unroll
                    for (int c = 0; c < OM_TW; ++c) {
                        const d2 a = f[c][kk];   // applied conjugated
                        mma3m(p1[c], p2[c], p3[c], a.x, -a.y, a.x - a.y, r.x, r.y, rs);
                    }
                }
            };
            gload(fa, 0);
            for (int s = 0; s < nst; s += 2) {
                gload(fb, s + 1);
                __builtin_amdgcn_sched_barrier(0);
                comp(fa, s);
                __builtin_amdgcn_sched_barrier(0);
                gload(fa, s + 2);
                __builtin_amdgcn_sched_barrier(0);
                if (s + 1 < nst) comp(fb, s + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // epilogue: lane l, register q: atom j0 + 16 c + (l >> 4) + 4 q, realisation l & 15
#pragma unroll
            for (int c = 0; c < OM_TW; ++c) {
                const int jt = j0 + 16 * c;
                if (jt < N) {   // (wave-uniform)
                    const uint32_t word = bm[(lane & 15) * OM_BMW + (jt >> 5)];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = jt + (lane >> 4) + 4 * q;
                        if (j < N && !((word >> (j & 31)) & 1u)) {
                            const d2 y = comb3m(p1[c][q], p2[c][q], p3[c][q]);
                            double P = y.x * y.x + y.y * y.y;
                            if (colscale) P *= colscale[j];
                            if (om_before(P, j, bv, bj)) {
                                bv = P;
                                bj = j;
                            }
                        }
                    }
                }
            }
        }
        // the wave's candidate per realisation: fold the four lanes of a column
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (om_before(ov, oj, bv, bj)) {
                bv = ov;
                bj = oj;
            }
        }
        if (lane < OM_RB) {
            wbv[w][lane] = bv;
            wbj[w][lane] = bj;
        }
        __syncthreads();

        // ================= selection and least-squares step: the group of realisation g
        if (active) {   // (group-uniform)
            double sv = wbv[0][g];
            int j = wbj[0][g];
#pragma unroll
            for (int v = 1; v < OM_WAVES; ++v)
                if (om_before(wbv[v][g], wbj[v][g], sv, j)) {
                    sv = wbv[v][g];
                    j = wbj[v][g];
                }
            if (j < 0) {
                active = false;   // no atom left to offer (cannot happen while k < kmax <= N)
            } else {
                // v = d_j, orthogonalised against q_0 .. q_{k-1} in sequence
                d2 v[OM_NU], qa[OM_NU];
                double a2 = 0.0;
#pragma unroll
                for (int u = 0; u < OM_NU; ++u) {
                    const int e = gl + OM_GL * u;
                    v[u] = make_double2(0.0, 0.0);
                    if (e < d) v[u] = D[(size_t)e * N + j];
                    a2 += cabs2(v[u]);
                }
                a2 = om_gsum(a2);
                auto qload = [&](d2(&q)[OM_NU], int i) {
#pragma unroll
                    for (int u = 0; u < OM_NU; ++u) {
                        const int e = gl + OM_GL * u;
                        q[u] = make_double2(0.0, 0.0);
                        if (e < d && i < k) q[u] = Qb[(size_t)i * d + e];
                    }
                };
                qload(qa, 0);
                for (int i = 0; i < k; ++i) {
                    d2 qn[OM_NU];
                    qload(qn, i + 1);
                    double pr = 0.0, pi = 0.0;
#pragma unroll
                    for (int u = 0; u < OM_NU; ++u) {
                        const d2 c = cmulc(qa[u], v[u]);
                        pr += c.x;
                        pi += c.y;
                    }
                    const d2 rho = make_double2(om_gsum(pr), om_gsum(pi));
#pragma unroll
                    for (int u = 0; u < OM_NU; ++u) {
                        v[u] = csub(v[u], cmul(rho, qa[u]));
                        qa[u] = qn[u];
                    }
                    if (gl == (i & (OM_GL - 1))) Fb[(size_t)k * kmax + i] = rho;
                }
                double n2 = 0.0;
#pragma unroll
                for (int u = 0; u < OM_NU; ++u) n2 += cabs2(v[u]);
                n2 = om_gsum(n2);
                if (!(n2 > OM_DEP * OM_DEP * a2)) {
                    stat |= ACE_ST_OMP_DEPENDENT;   // the atom is not added
                    active = false;
                } else {
                    const double nv = sqrt(n2);
                    double pr = 0.0, pi = 0.0;
#pragma unroll
                    for (int u = 0; u < OM_NU; ++u) {
                        const int e = gl + OM_GL * u;
                        v[u] = make_double2(v[u].x / nv, v[u].y / nv);
                        qa[u] = make_double2(0.0, 0.0);
                        if (e < d) {
                            Qb[(size_t)k * d + e] = v[u];
                            qa[u] = Rs[g * ST + e];
                        }
                        const d2 c = cmulc(v[u], qa[u]);
                        pr += c.x;
                        pi += c.y;
                    }
                    const d2 z = make_double2(om_gsum(pr), om_gsum(pi));
                    double r2 = 0.0;
#pragma unroll
                    for (int u = 0; u < OM_NU; ++u) {
                        const int e = gl + OM_GL * u;
                        qa[u] = csub(qa[u], cmul(z, v[u]));
                        if (e < d) {
                            Rs[g * ST + e] = qa[u];
                            r2 += cabs2(qa[u]);
                        }
                    }
                    rn = sqrt(om_gsum(r2));
                    if (gl == (k & (OM_GL - 1))) {
                        Fb[(size_t)k * kmax + k] = make_double2(nv, 0.0);
                        zb[k] = z;
                        idx[(size_t)b * kmax + k] = j;
                    }
                    if (gl == 0) bm[g * OM_BMW + (j >> 5)] |= 1u << (j & 31);
                    ++k;
                    active = k < kmax && rn > tol;
                }
            }
            if (!active)
                for (int e = gl; e < DP; e += OM_GL) Rs[g * ST + e] = make_double2(0.0, 0.0);
        }
    }

    // ---------------- outputs: back substitution R c = z (row i on lane i & 31, which wrote it), the tails, x
    if (!live) return;
    for (int i = k - 1; i >= 0; --i) {
        const int owner = i & (OM_GL - 1);
        d2 c = make_double2(0.0, 0.0);
        if (gl == owner) {
            const d2 zi = zb[i];
            const double rii = Fb[(size_t)i * kmax + i].x;
            c = make_double2(zi.x / rii, zi.y / rii);
            coef[(size_t)b * kmax + i] = c;
        }
        c.x = __shfl(c.x, owner, OM_GL);
        c.y = __shfl(c.y, owner, OM_GL);
        for (int r = gl; r < i; r += OM_GL) zb[r] = csub(zb[r], cmul(Fb[(size_t)i * kmax + r], c));
    }
    for (int i = k + gl; i < kmax; i += OM_GL) {
        idx[(size_t)b * kmax + i] = -1;
        coef[(size_t)b * kmax + i] = make_double2(0.0, 0.0);
    }
    if (gl == 0) {
        count[b] = k;
        resnorm[b] = rn;
        if (status) status[b] = stat;
    }
    if (xout) {   // zeros off the support (the bitmap tells), the coefficients on it (written above by this thread)
        for (int j = gl; j < N; j += OM_GL)
            if (!((bm[g * OM_BMW + (j >> 5)] >> (j & 31)) & 1u)) xout[(size_t)b * N + j] = make_double2(0.0, 0.0);
        for (int i = gl; i < k; i += OM_GL) xout[(size_t)b * N + idx[(size_t)b * kmax + i]] = coef[(size_t)b * kmax + i];
    }
}

int om_check_args(int batch, int d, int N, int kmax, double tol, const double* D, const double* Y, const int32_t* idx,
                  const double* coef, const int32_t* count, const double* resnorm) {
    if (batch < 1) return fail(ACE_ERR_ARG, "omp: batch %d < 1", batch);
    if (d < 1 || d > OM_DMAX) return fail(d < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "omp: d %d outside 1..%d", d, OM_DMAX);
    if (N < 1 || N > OM_NMAX) return fail(N < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "omp: N %d outside 1..%d", N, OM_NMAX);
    if (kmax < 1 || kmax > d || kmax > N)
        return fail(ACE_ERR_ARG, "omp: kmax %d outside 1..min(d = %d, N = %d, %d)", kmax, d, N, OM_DMAX);
    if (!(tol >= 0.0)) return fail(ACE_ERR_ARG, "omp: tol %g is not >= 0", tol);
    if (!D || !Y || !idx || !coef || !count || !resnorm)
        return fail(ACE_ERR_ARG, "omp: NULL %s", !D ? "D" : !Y ? "Y" : !idx ? "idx" : !coef ? "coef" : !count ? "count" : "resnorm");
    return ACE_OK;
}

size_t om_ws_bytes(int batch, int d, int kmax) {
    return (((size_t)batch * om_ws_entries(d, kmax) * sizeof(d2) + 255) & ~(size_t)255) + 256;   // (the base is rounded up to 256 B)
}

}  // namespace

size_t omp_request_bytes(int d) { return om_lds_bytes(d < 1 ? 1 : d > OM_DMAX ? OM_DMAX : d); }

}  // namespace ace

using namespace ace;

extern "C" size_t ace_omp_workspace_size(int batch, int d, int N, int kmax) {
    if (batch < 1 || d < 1 || d > OM_DMAX || N < 1 || N > OM_NMAX || kmax < 1 || kmax > d || kmax > N) return 0;
    return om_ws_bytes(batch, d, kmax);
}

extern "C" int ace_omp_solve_batch(int batch, int d, int N, int kmax, double tol, const double* D, const double* colscale,
                                   const double* Y, int32_t* idx, double* coef, int32_t* count, double* resnorm,
                                   uint32_t* status, double* x, void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(om_check_args(batch, d, N, kmax, tol, D, Y, idx, coef, count, resnorm));
    const size_t need = om_ws_bytes(batch, d, kmax);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "omp: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    // up to 98624 B of dynamic LDS, past the 64 KiB default: the kernel's derived budget decides (no fallback)
    const void* const kern = reinterpret_cast<const void*>(&omp_kernel);
    const size_t lds = om_lds_bytes(d);
    if (!lds_ok(kern, lds))
        return fail(ACE_ERR_UNSUPPORTED, "omp: omp_kernel needs %zu B of dynamic LDS, budget %zu B", lds, lds_dyn_budget(kern));
    const int nblk = (batch + OM_RB - 1) / OM_RB;
    hipLaunchKernelGGL(omp_kernel, dim3(nblk), dim3(OM_NT), lds, (hipStream_t)stream, batch, d, N, kmax, tol, (const d2*)D,
                       colscale, (const d2*)Y, idx, (d2*)coef, count, resnorm, status, (d2*)x, (d2*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255));
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_omp_solve_host(int batch, int d, int N, int kmax, double tol, const double* D, const double* colscale,
                                  const double* Y, int32_t* idx, double* coef, int32_t* count, double* resnorm,
                                  uint32_t* status, double* x) {
    g_err.clear();
    ACE_TRY(om_check_args(batch, d, N, kmax, tol, D, Y, idx, coef, count, resnorm));
    const size_t B = batch, wsb = om_ws_bytes(batch, d, kmax);
    DevScope dev;
    double *dD, *dcs = nullptr, *dY, *dcoef, *dres, *dx = nullptr;
    int32_t *didx, *dcount;
    uint32_t* dst;
    char* dws;
    ACE_TRY(dev.put(&dD, D, 2 * (size_t)d * N));
    if (colscale) ACE_TRY(dev.put(&dcs, colscale, (size_t)N));
    ACE_TRY(dev.put(&dY, Y, 2 * B * d));
    ACE_TRY(dev.alloc(&didx, B * kmax));
    ACE_TRY(dev.alloc(&dcoef, 2 * B * kmax));
    ACE_TRY(dev.alloc(&dcount, B));
    ACE_TRY(dev.alloc(&dres, B));
    ACE_TRY(dev.alloc(&dst, B));
    if (x) ACE_TRY(dev.alloc(&dx, 2 * B * N));
    ACE_TRY(dev.alloc(&dws, wsb));
    ACE_TRY(ace_omp_solve_batch(batch, d, N, kmax, tol, dD, dcs, dY, didx, dcoef, dcount, dres, dst, dx, dws, wsb, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(idx, didx, B * kmax));
    ACE_TRY(dev.get(coef, dcoef, 2 * B * kmax));
    ACE_TRY(dev.get(count, dcount, B));
    ACE_TRY(dev.get(resnorm, dres, B));
    ACE_TRY(dev.get(status, dst, B));
    return dev.get(x, dx, 2 * B * N);
}
