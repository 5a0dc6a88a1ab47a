// Batched Bayesian A-optimal probe selection (Bayes_Beam.m -> bayesAopt_complex.m:105-254 with A = I, K = kdiag I,
// no fixed rows): a Fedorov row exchange that picks nrows rows of a candidate codebook F [P][n] to minimise
// trace((X^H X + K)^-1), the posterior variance of the channel estimate.  Designs of one call share F; each has its
// own row count and start rows.
//
// Notation: x_i = f_i^H (the candidates as columns), Minv = (X^H X + K)^-1 (Hermitian n x n), g_i = x_i^H Minv x_i,
// t_i = ||Minv x_i||^2, Acrit = trace(Minv).  One step, for row r of the design with x its current candidate:
//
//   u = Minv x;  w = 1 / (1 - Re x^H u);  v = Minv u;  beta = ||u||^2
//   every candidate i:  p_i = u^H x_i, q_i = v^H x_i
//       g'_i = g_i + w |p_i|^2;  W_i = 1 / (1 + g'_i);  t'_i = t_i + 2 w Re(q_i conj p_i) + beta w^2 |p_i|^2
//       ad_i = w beta - W_i t'_i
//   j = first index of min ad, a = ad_j;  switch iff a < acutoff or row r is unassigned
//   on a switch:  Acrit += a, rowlist[r] = j,  Ninv = Minv + w u u^H
//       u+ = Ninv x_j = Minv x_j + w (u^H x_j) u;  w+ = W_j;  v+ = Ninv u+ = Minv u+ + w (u^H u+) u;  beta+ = ||u+||^2
//       p+_i = u+^H x_i, q+_i = v+^H x_i
//       Minv = Minv + w u u^H - w+ u+ u+^H
//       g_i = g'_i - w+ |p+_i|^2;  t_i = t'_i - 2 w+ Re(q+_i conj p+_i) + beta+ w+^2 |p+_i|^2
//
// Passes over the rows repeat while some row switched and iter < maxiter.  (The reference also forms
// NinvF = Ninv F^H, :233, and never reads it; it is not formed.)
//
// Kernels.  A step is ten launches over all designs of the call; the stream orders them, nothing spins across
// work-groups, there are no atomics and every sum has a fixed order.
//   mv<0> u, scal1 (w, beta, the singularity test), mv<1> v, sweep<false>, decide,
//   mv<2> u+, scal2 (beta+, u^H u+), mv<3> v+, sweep<true>, rank2.
// The switch decision stays on the device: decide leaves a per-design flag, and the launches after it do nothing
// for a design that did not switch, has stopped or has fewer rows than r.  The host reads one word per pass (the
// number of designs still running).
//
// Candidate sweep (the hot part): sum_k V[rho][k] F[i][k] for the 16 vectors rho (u and v of up to AO_DG = 8
// designs) against every candidate i is one complex product, P x n x 16, on v_mfma_f64_16x16x4_f64 in the 4M form
// (cmma of ace_mfma.hpp: each part of a result is one chain of real products, so its error is bounded
// componentwise, and the values decide an argmin with small margins).  p_i is the conjugate of the u entry.  A
// work-group (4 waves) owns a tile of 16 candidates; its waves split k in chunks of 16 (wave w: chunks w, w + 4,
// ...), each lane loading 4 consecutive entries (64 B) of its candidate row and of its vector per chunk straight
// from global memory: within a chunk, k-step kk of lane l carries k = 16 c + 4 (l >> 4) + kk for both operands, a
// fixed permutation of the sum.  The four partial tiles are added through LDS in wave order.  The epilogue
// (wave 0) forms g', W, t' and ad and folds the running argmin under the strict order "smaller value, or equal
// value and smaller index" over the 16 lanes of a design; one (value, index) pair per tile and design goes to
// memory, and decide folds the pairs.  The P-long ad is never written.  Rows k >= n and candidates i >= P are
// masked at the loads.  Equal candidate rows go through the same chain of operations whatever tile they stand in,
// so their values are equal bit for bit and the smaller index wins.
//
// Minv side: the four matrix-vector products read Minv once each, one wave per row (lane partial sums over
// k = lane + 64 j, then a butterfly); the rank-two update rewrites it once.  Its entry (i, k) and (k, i) are formed
// from the same products in the same order (the imaginary part as a difference of two rounded products), so Minv
// stays exactly Hermitian.  The start takes the smaller of two systems, by the design's own row count nr: nr >= n
// forms X^H X / kdiag (upper triangle, mirrored) and inverts I + X^H X / kdiag; nr < n inverts the nr x nr matrix
// I + X X^H / kdiag = S^-1 and forms Minv = (I - X^H S X / kdiag) / kdiag (Woodbury: at n = 1024 the elimination of
// the n x n system, one work-group per design, took two thirds of a call).  The elimination is launch_inv_ipk's
// Gauss-Jordan with the order read per design (ao_inv_kernel); the result is symmetrised and scaled by 1 / kdiag.
// g and t of the start are one more product on the matrix cores (ao_gt_kernel: Minv against the conjugated
// candidates, reduced per candidate in a fixed order).
//
// Batch invariance.  A design's outputs are a function of (F, its nrows, its init, cfg) alone: a design's rows of
// the MFMA tiles do not depend on the other rows, the tile and chunk walk depends on P and n only, all sums have
// a fixed order and the argmin is order-free.  Minv_out is a copy of the working matrix.
//
// Resources as compiled: DESIGN.md §4j.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

namespace ace {
namespace {

constexpr int AO_NMAX = 1024;     // largest n
constexpr int AO_PMAX = 65536;    // largest P
constexpr int AO_RMAX = 4096;     // largest nrows
constexpr int AO_DG = 8;          // designs per sweep tile (two vectors each: the 16 rows of an MFMA tile)
constexpr int AO_WAVES = 4;
constexpr int AO_NT = 64 * AO_WAVES;

struct AoState {   // per design, in the workspace
    double w, beta, wp, betap;   // w, beta of the removal; w+, beta+ of the insertion
    d2 c, c2;                    // u^H x_j, u^H u+
    double acrit0, acrit;
    int32_t live;                // still running
    int32_t sw;                  // the current step switched
    int32_t made;                // some row switched in the current pass
    int32_t iters, switches, j, nr, pad_;
    uint32_t status, pad2_[3];
};
static_assert(sizeof(AoState) % 16 == 0, "AoState alignment");

struct AoBufs {
    d2* Minv;          // [designs][n][n]
    double *g, *t;     // [designs][P]
    double *gn, *tn;   // [designs][P]: g', t' of the current step
    d2 *U, *V, *UP, *VP;   // [designs][n]
    double* pval;      // [designs][ntile]: the tiles' argmin candidates
    int32_t* pidx;
    int32_t* cur;      // [designs][nrows_max]: the candidate each design row holds
    AoState* st;       // [designs]
    int32_t* nlive;    // [1]
    d2* T;             // [designs][min(nrows_max, n)][n]: S X of the start (designs with fewer rows than n)
};

constexpr int ao_ntile(int P) { return (P + 15) / 16; }

void ao_carve(Carver& cv, int designs, int P, int n, int nrows_max, AoBufs* b) {
    const size_t D = designs;
    b->Minv = cv.take<d2>(D * n * n * sizeof(d2));
    b->g = cv.take<double>(D * P * sizeof(double));
    b->t = cv.take<double>(D * P * sizeof(double));
    b->gn = cv.take<double>(D * P * sizeof(double));
    b->tn = cv.take<double>(D * P * sizeof(double));
    b->U = cv.take<d2>(D * n * sizeof(d2));
    b->V = cv.take<d2>(D * n * sizeof(d2));
    b->UP = cv.take<d2>(D * n * sizeof(d2));
    b->VP = cv.take<d2>(D * n * sizeof(d2));
    b->pval = cv.take<double>(D * ao_ntile(P) * sizeof(double));
    b->pidx = cv.take<int32_t>(D * ao_ntile(P) * sizeof(int32_t));
    b->cur = cv.take<int32_t>(D * nrows_max * sizeof(int32_t));
    b->st = cv.take<AoState>(D * sizeof(AoState));
    b->nlive = cv.take<int32_t>(sizeof(int32_t));
    b->T = cv.take<d2>(D * (nrows_max < n ? nrows_max : n) * n * sizeof(d2));
}

// the strict order of the argmin: a candidate (value a, index ia >= 0) goes before (b, ib)
__device__ __forceinline__ bool ao_before(double a, int ia, double b, int ib) {
    return ia >= 0 && (ib < 0 || a < b || (a == b && ia < ib));
}

__device__ __forceinline__ bool ao_runs(const AoState& s, int r) { return s.live && r < s.nr; }

// ---------------------------------------------------------------- start
// rows and counters of every design; nrows and init are clamped into their ranges, so nothing is read out of bounds
__global__ __launch_bounds__(256) void ao_prep_kernel(int P, int nrows_max, const int32_t* __restrict__ nrows,
                                                      const int32_t* __restrict__ init, int32_t* __restrict__ cur,
                                                      int32_t* __restrict__ rowlist, AoState* __restrict__ st) {
    const int d = blockIdx.x;
    const int nr = min(max(nrows[d], 1), nrows_max);
    for (int r = threadIdx.x; r < nrows_max; r += 256) {
        cur[(size_t)d * nrows_max + r] = min(max(init[(size_t)d * nrows_max + r], 0), P - 1);
        rowlist[(size_t)d * nrows_max + r] = -1;
    }
    if (threadIdx.x == 0) {
        AoState s = {};
        s.live = 1;
        s.nr = nr;
        s.j = -1;
        st[d] = s;
    }
}

// The start's inverse takes the smaller of two systems, by the design's own row count nr (so a design's result does
// not depend on the batch it is in): nr >= n inverts I + X^H X / kdiag (n x n) directly; nr < n goes through
// S = (I + X X^H / kdiag)^-1 (nr x nr) and Minv = (I - X^H S X / kdiag) / kdiag (Woodbury).
__device__ __forceinline__ bool ao_small(const AoState& s, int n) { return s.nr < n; }

// G = X^H X / kdiag (n x n), or X X^H / kdiag (nr x nr, leading dimension nr) for a design with nr < n: the upper
// triangle, mirrored (exactly Hermitian); into the design's Minv buffer
__global__ __launch_bounds__(256) void ao_gram_kernel(int n, int nrows_max, double kdiag, const d2* __restrict__ F,
                                                      const int32_t* __restrict__ cur, const AoState* __restrict__ st,
                                                      d2* __restrict__ Minv) {
    const int d = blockIdx.z;
    const int k = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
    const int nr = st[d].nr;
    const bool small = ao_small(st[d], n);
    const int m = small ? nr : n;
    if (i >= m || k >= m || k < i) return;
    const int32_t* c = cur + (size_t)d * nrows_max;
    double sr = 0.0, si = 0.0;
    if (small) {
        const d2 *fi = F + (size_t)c[i] * n, *fk = F + (size_t)c[k] * n;
        for (int e = 0; e < n; ++e) {
            const d2 a = fi[e], b = fk[e];   // a conj(b)
            sr += a.x * b.x + a.y * b.y;
            si += a.y * b.x - a.x * b.y;
        }
    } else {
        for (int r = 0; r < nr; ++r) {
            const d2* f = F + (size_t)c[r] * n;
            const d2 a = f[i], b = f[k];   // conj(a) b
            sr += a.x * b.x + a.y * b.y;
            si += a.x * b.y - a.y * b.x;
        }
    }
    sr /= kdiag;
    si = i == k ? 0.0 : si / kdiag;
    d2* G = Minv + (size_t)d * n * n;
    G[(size_t)i * m + k] = make_double2(sr, si);
    G[(size_t)k * m + i] = make_double2(sr, -si);
}

// (I + G)^-1 in place, G Hermitian positive semidefinite of order m = nr (nr < n) or n: Gauss-Jordan without pivoting,
// one work-group per design (launch_inv_ipk's elimination with the order read per design)
__global__ __launch_bounds__(1024) void ao_inv_kernel(int n, const AoState* __restrict__ st, d2* __restrict__ Minv) {
    extern __shared__ __align__(16) unsigned char ao_lds[];
    d2* rowk = reinterpret_cast<d2*>(ao_lds);
    const int d = blockIdx.x, m = ao_small(st[d], n) ? st[d].nr : n;
    d2* colk = rowk + m;
    d2* G = Minv + (size_t)d * n * n;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int i = t; i < m; i += nt) G[(size_t)i * m + i].x += 1.0;
    __syncthreads();
    for (int k = 0; k < m; ++k) {
        const d2 p = G[(size_t)k * m + k];
        const double den = p.x * p.x + p.y * p.y;
        const d2 pinv = make_double2(p.x / den, -p.y / den);
        for (int j = t; j < m; j += nt) {
            const d2 a = (j == k) ? make_double2(1.0, 0.0) : G[(size_t)k * m + j];
            rowk[j] = cmul(a, pinv);
            colk[j] = (j == k) ? make_double2(0.0, 0.0) : G[(size_t)j * m + k];
        }
        __syncthreads();
        for (int e = t; e < m * m; e += nt) {
            const int i = e / m, j = e - i * m;
            d2* gij = &G[(size_t)i * m + j];
            if (i == k) {
                *gij = rowk[j];
            } else {
                const d2 base = (j == k) ? make_double2(0.0, 0.0) : *gij;
                *gij = csub(base, cmul(colk[i], rowk[j]));
            }
        }
        __syncthreads();
    }
}

// nr < n: T = S X (nr x n), S in the design's Minv buffer (leading dimension nr).  Grid (n / 256, n, designs).
__global__ __launch_bounds__(256) void ao_wood_t_kernel(int n, int nrows_max, int trows, const d2* __restrict__ F,
                                                        const int32_t* __restrict__ cur, const AoState* __restrict__ st,
                                                        const d2* __restrict__ Minv, d2* __restrict__ T) {
    const int d = blockIdx.z, r = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int nr = st[d].nr;
    if (!ao_small(st[d], n) || r >= nr || k >= n) return;
    const d2* S = Minv + (size_t)d * n * n + (size_t)r * nr;
    const int32_t* c = cur + (size_t)d * nrows_max;
    d2 acc = make_double2(0.0, 0.0);
    for (int s = 0; s < nr; ++s) acc = cadd(acc, cmul(S[s], F[(size_t)c[s] * n + k]));
    T[((size_t)d * trows + r) * n + k] = acc;
}

// nr < n: Minv = I - X^H T / kdiag (ao_herm_kernel symmetrises and divides by kdiag).  Grid (n / 256, n, designs).
__global__ __launch_bounds__(256) void ao_wood_m_kernel(int n, int nrows_max, int trows, double kdiag,
                                                        const d2* __restrict__ F, const int32_t* __restrict__ cur,
                                                        const AoState* __restrict__ st, const d2* __restrict__ T,
                                                        d2* __restrict__ Minv) {
    const int d = blockIdx.z, i = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
    const int nr = st[d].nr;
    if (!ao_small(st[d], n) || k >= n) return;
    const int32_t* c = cur + (size_t)d * nrows_max;
    const d2* Td = T + (size_t)d * trows * n;
    d2 acc = make_double2(0.0, 0.0);
    for (int r = 0; r < nr; ++r) acc = cadd(acc, cmulc(F[(size_t)c[r] * n + i], Td[(size_t)r * n + k]));
    Minv[((size_t)d * n + i) * n + k] = make_double2((i == k ? 1.0 : 0.0) - acc.x / kdiag, -acc.y / kdiag);
}

// Minv <- (Minv + Minv^H) / (2 kdiag), the diagonal real
__global__ __launch_bounds__(256) void ao_herm_kernel(int n, double kdiag, d2* __restrict__ Minv) {
    const int d = blockIdx.z;
    const int k = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= n || k >= n || k < i) return;
    d2* G = Minv + (size_t)d * n * n;
    const d2 a = G[(size_t)i * n + k], b = G[(size_t)k * n + i];
    const double hr = 0.5 * (a.x + b.x) / kdiag, hi = i == k ? 0.0 : 0.5 * (a.y - b.y) / kdiag;
    G[(size_t)i * n + k] = make_double2(hr, hi);
    G[(size_t)k * n + i] = make_double2(hr, -hi);
}

// Acrit = trace(Minv) of the start
__global__ __launch_bounds__(256) void ao_trace_kernel(int n, const d2* __restrict__ Minv, AoState* __restrict__ st) {
    __shared__ double sh[16];
    const int d = blockIdx.x;
    const d2* G = Minv + (size_t)d * n * n;
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += 256) v[0] += G[(size_t)i * n + i].x;
    block_sum(v, sh);
    if (threadIdx.x == 0) st[d].acrit0 = st[d].acrit = v[0];
}

// ---------------------------------------------------------------- the 16 x 16 complex tile on the matrix cores
// (cr, ci) += D[row][col] = sum_k A[row][k] B[col][k] (B conjugated with CONJB) over the chunks c0, c0 + cs, ... of
// 16 k.  ap / bp: the lane's operand rows, A row l & 15 and B row l & 15 (nullptr: a zero row).  Lane l carries
// k = 16 c + 4 (l >> 4) + kk in k-step kk of chunk c; result: lane l, register q holds D[(l >> 4) + 4 q][l & 15].
// The chunk bounds are wave-uniform: every MFMA runs with all lanes.
template <bool CONJB>
__device__ __forceinline__ void ao_tile(const d2* ap, const d2* bp, int n, int c0, int cs, int lane, d4v& cr, d4v& ci) {
    const int nch = (n + 15) / 16, ks = 4 * (lane >> 4);
    const d2 zero = make_double2(0.0, 0.0);
    auto load = [&](d2(&a)[4], d2(&b)[4], int c) {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const int k = 16 * c + ks + kk;
            a[kk] = (ap && k < n) ? ap[k] : zero;
            b[kk] = (bp && k < n) ? bp[k] : zero;
        }
    };
    d2 a0[4], b0[4], a1[4], b1[4];
    if (c0 < nch) load(a0, b0, c0);
    for (int c = c0; c < nch; c += cs) {
        const bool more = c + cs < nch;
        if (more) load(a1, b1, c + cs);   // the next chunk's loads are issued ahead of this chunk's MFMAs
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            d2 b = b0[kk];
            if (CONJB) b.y = -b.y;
            cmma(cr, ci, a0[kk], b);
        }
        if (more) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a0[kk] = a1[kk];
                b0[kk] = b1[kk];
            }
        }
    }
}

// g_i = x_i^H Minv x_i and t_i = ||Minv x_i||^2 of the start.  Grid (tiles of 16 candidates, designs); wave w walks
// the row tiles w, w + 4, ... of Minv with the whole k range each: Y[row][i] = sum_k Minv[row][k] conj(F[i][k]).
__global__ __launch_bounds__(AO_NT) void ao_gt_kernel(int P, int n, const d2* __restrict__ F, const d2* __restrict__ Minv,
                                                      double* __restrict__ g, double* __restrict__ t) {
    __shared__ double part[AO_WAVES][2][16];
    const int d = blockIdx.y, i0 = blockIdx.x * 16;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const d2* G = Minv + (size_t)d * n * n;
    const int cand = i0 + (lane & 15);
    const d2* bp = cand < P ? F + (size_t)cand * n : nullptr;
    double gs = 0.0, ts = 0.0;
    for (int rt = w; rt < (n + 15) / 16; rt += AO_WAVES) {
        const int row = rt * 16 + (lane & 15);
        const d2* ap = row < n ? G + (size_t)row * n : nullptr;
        d4v cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        ao_tile<true>(ap, bp, n, 0, 1, lane, cr, ci);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = rt * 16 + (lane >> 4) + 4 * q;
            if (e < n && bp) {
                const d2 f = bp[e];   // conj(x_i[e]) = F[i][e]
                gs += f.x * cr[q] - f.y * ci[q];
                ts += cr[q] * cr[q] + ci[q] * ci[q];
            }
        }
    }
    gs += __shfl_xor(gs, 16, 64);
    gs += __shfl_xor(gs, 32, 64);
    ts += __shfl_xor(ts, 16, 64);
    ts += __shfl_xor(ts, 32, 64);
    if (lane < 16) {
        part[w][0][lane] = gs;
        part[w][1][lane] = ts;
    }
    __syncthreads();
    if (threadIdx.x < 16 && cand < P) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int v = 0; v < AO_WAVES; ++v) {
            a += part[v][0][threadIdx.x];
            b += part[v][1][threadIdx.x];
        }
        g[(size_t)d * P + cand] = a;
        t[(size_t)d * P + cand] = b;
    }
}

// ---------------------------------------------------------------- Minv side
// MODE 0: u = Minv x (x the candidate row r holds);  1: v = Minv u;  2: u+ = Minv x_j + w (u^H x_j) u;
// 3: v+ = Minv u+ + w (u^H u+) u.  One wave per row of Minv.
template <int MODE>
__global__ __launch_bounds__(AO_NT) void ao_mv_kernel(int n, int nrows_max, int r, const d2* __restrict__ F,
                                                      const int32_t* __restrict__ cur, const AoState* __restrict__ st,
                                                      const d2* __restrict__ Minv, const d2* __restrict__ U,
                                                      const d2* __restrict__ UP, d2* __restrict__ out) {
    const int d = blockIdx.y;
    const AoState s = st[d];
    if (!ao_runs(s, r) || (MODE >= 2 && !s.sw)) return;
    const int lane = threadIdx.x & 63, i = blockIdx.x * AO_WAVES + (threadIdx.x >> 6);
    if (i >= n) return;
    const d2* row = Minv + ((size_t)d * n + i) * n;
    const d2* x = MODE == 1 ? U + (size_t)d * n : MODE == 3 ? UP + (size_t)d * n
                                                            : F + (size_t)cur[(size_t)d * nrows_max + r] * n;
    double ar = 0.0, ai = 0.0;
    for (int k = lane; k < n; k += 64) {
        const d2 m = row[k];
        d2 v = x[k];
        if (MODE == 0 || MODE == 2) v.y = -v.y;   // x = f^H
        ar += m.x * v.x - m.y * v.y;
        ai += m.x * v.y + m.y * v.x;
    }
    ar = wave_sum(ar);
    ai = wave_sum(ai);
    if (lane == 0) {
        d2 y = make_double2(ar, ai);
        if (MODE >= 2) {
            const d2 c = MODE == 2 ? s.c : s.c2;
            y = cadd(y, cmul(cscale(c, s.w), U[(size_t)d * n + i]));
        }
        out[(size_t)d * n + i] = y;
    }
}

// w = 1 / (1 - Re x^H u), beta = ||u||^2.  A design whose 1 - Re x^H u is not positive and finite stops here with
// its rows as they stand (ACE_ST_AOPT_SINGULAR).
__global__ __launch_bounds__(256) void ao_scal1_kernel(int n, int nrows_max, int r, const d2* __restrict__ F,
                                                       const int32_t* __restrict__ cur, const d2* __restrict__ U,
                                                       AoState* __restrict__ st) {
    __shared__ double sh[32];
    const int d = blockIdx.x;
    if (!ao_runs(st[d], r)) return;
    const d2* f = F + (size_t)cur[(size_t)d * nrows_max + r] * n;
    const d2* u = U + (size_t)d * n;
    double v[2] = {0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += 256) {
        const d2 a = f[k], b = u[k];
        v[0] += a.x * b.x - a.y * b.y;   // Re x^H u = Re sum_k f_k u_k
        v[1] += cabs2(b);
    }
    block_sum(v, sh);
    if (threadIdx.x == 0) {
        const double den = 1.0 - v[0];
        if (!(den > 0.0) || !isfinite(den) || !isfinite(v[1])) {
            st[d].status |= ACE_ST_AOPT_SINGULAR;
            st[d].live = 0;
        } else {
            st[d].w = 1.0 / den;
            st[d].beta = v[1];
        }
    }
}

// beta+ = ||u+||^2 and u^H u+ (for v+)
__global__ __launch_bounds__(256) void ao_scal2_kernel(int n, int r, const d2* __restrict__ U, const d2* __restrict__ UP,
                                                       AoState* __restrict__ st) {
    __shared__ double sh[48];
    const int d = blockIdx.x;
    if (!ao_runs(st[d], r) || !st[d].sw) return;
    const d2* u = U + (size_t)d * n;
    const d2* up = UP + (size_t)d * n;
    double v[3] = {0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < n; k += 256) {
        const d2 a = u[k], b = up[k];
        const d2 c = cmulc(a, b);
        v[0] += cabs2(b);
        v[1] += c.x;
        v[2] += c.y;
    }
    block_sum(v, sh);
    if (threadIdx.x == 0) {
        st[d].betap = v[0];
        st[d].c2 = make_double2(v[1], v[2]);
    }
}

// Minv += w u u^H - w+ u+ u+^H; entries (i, k) and (k, i) come out as exact conjugates
__global__ __launch_bounds__(256) void ao_rank2_kernel(int n, int r, const AoState* __restrict__ st,
                                                       const d2* __restrict__ U, const d2* __restrict__ UP,
                                                       d2* __restrict__ Minv) {
#pragma clang fp contract(off)   // every product rounded on its own: a fused multiply-add would break the symmetry
    const int d = blockIdx.z;
    const AoState s = st[d];
    if (!ao_runs(s, r) || !s.sw) return;
    const int k = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (k >= n) return;
    const d2 ui = U[(size_t)d * n + i], uk = U[(size_t)d * n + k];
    const d2 pi = UP[(size_t)d * n + i], pk = UP[(size_t)d * n + k];
    // z conj(y): re = z.x y.x + z.y y.y, im = z.y y.x - z.x y.y
    const double r1 = ui.x * uk.x + ui.y * uk.y, i1 = ui.y * uk.x - ui.x * uk.y;
    const double r2 = pi.x * pk.x + pi.y * pk.y, i2 = pi.y * pk.x - pi.x * pk.y;
    d2* m = Minv + ((size_t)d * n + i) * n + k;
    d2 e = *m;
    e.x = (e.x + s.w * r1) - s.wp * r2;
    e.y = (e.y + s.w * i1) - s.wp * i2;
    *m = e;
}

// ---------------------------------------------------------------- candidate sweep
// Grid (tiles of 16 candidates, groups of AO_DG designs).  Vector row rho = s + 4 q of the tile (s = rho & 3,
// q = rho >> 2) is design AO_DG grp + s + 4 (q >> 1), its u (q even) or v (q odd): the lane of the result that
// holds candidate l & 15 then has u and v of the designs s = l >> 4 and s + 4 in its four registers.
// SECOND: the insertion's sweep (u+, v+; g, t from g', t'), for the designs that switched.
template <bool SECOND>
__global__ __launch_bounds__(AO_NT) void ao_sweep_kernel(int designs, int P, int n, int r, const d2* __restrict__ F,
                                                         const AoState* __restrict__ st, const d2* __restrict__ Uv,
                                                         const d2* __restrict__ Vv, double* __restrict__ g,
                                                         double* __restrict__ t, double* __restrict__ gn,
                                                         double* __restrict__ tn, double* __restrict__ pval,
                                                         int32_t* __restrict__ pidx) {
    __shared__ double part[AO_WAVES - 1][8][64];
    const int grp = blockIdx.y, tile = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    auto runs = [&](int d) {
        if (d >= designs) return false;
        const AoState& s = st[d];
        return ao_runs(s, r) && (!SECOND || s.sw != 0);
    };
    bool any = false;
    for (int e = 0; e < AO_DG; ++e) any |= runs(AO_DG * grp + e);
    if (!any) return;   // (block-uniform)

    const int rho = lane & 15, q0 = rho >> 2;
    const int da = AO_DG * grp + (rho & 3) + 4 * (q0 >> 1);
    const d2* ap = runs(da) ? ((q0 & 1) ? Vv : Uv) + (size_t)da * n : nullptr;
    const int cand = tile * 16 + (lane & 15);
    const d2* bp = cand < P ? F + (size_t)cand * n : nullptr;
    d4v cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
    ao_tile<false>(ap, bp, n, w, AO_WAVES, lane, cr, ci);
    if (w > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            part[w - 1][q][lane] = cr[q];
            part[w - 1][4 + q][lane] = ci[q];
        }
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int v = 0; v < AO_WAVES - 1; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cr[q] += part[v][q][lane];
            ci[q] += part[v][4 + q][lane];
        }
    // epilogue: candidate `cand`, designs AO_DG grp + (lane >> 4) + 4 h; sp = conj(p), sq = conj(q) of the text
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int d = AO_DG * grp + (lane >> 4) + 4 * h;
        const bool on = runs(d);   // (uniform over the 16 lanes of a design)
        double ad = 0.0;
        int idx = -1;
        if (on && cand < P) {
            const AoState& s = st[d];
            const double pr = cr[2 * h], pi = ci[2 * h], qr = cr[2 * h + 1], qi = ci[2 * h + 1];
            const double ap2 = pr * pr + pi * pi, rqp = qr * pr + qi * pi;
            const size_t o = (size_t)d * P + cand;
            if (!SECOND) {
                const double wv = s.w, gp = g[o] + wv * ap2, W = 1.0 / (1.0 + gp);
                const double tp = t[o] + 2.0 * wv * rqp + s.beta * wv * wv * ap2;
                gn[o] = gp;
                tn[o] = tp;
                ad = wv * s.beta - W * tp;
                if (ad == ad) idx = cand;   // (a NaN is no candidate)
            } else {
                const double wv = s.wp;
                g[o] = gn[o] - wv * ap2;
                t[o] = tn[o] - 2.0 * wv * rqp + s.betap * wv * wv * ap2;
            }
        }
        if (!SECOND) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const double ov = __shfl_xor(ad, o, 64);
                const int oi = __shfl_xor(idx, o, 64);
                if (ao_before(ov, oi, ad, idx)) {
                    ad = ov;
                    idx = oi;
                }
            }
            if (on && (lane & 15) == 0) {
                pval[(size_t)d * gridDim.x + tile] = ad;
                pidx[(size_t)d * gridDim.x + tile] = idx;
            }
        }
    }
}

// The argmin over the tiles' candidates, the switch decision and, on a switch, w+ = W_j and u^H x_j (for u+)
__global__ __launch_bounds__(256) void ao_decide_kernel(int P, int n, int ntile, int nrows_max, int r, double acutoff,
                                                        const d2* __restrict__ F, const d2* __restrict__ U,
                                                        const double* __restrict__ gn, const double* __restrict__ pval,
                                                        const int32_t* __restrict__ pidx, int32_t* __restrict__ cur,
                                                        int32_t* __restrict__ rowlist, AoState* __restrict__ st) {
    __shared__ double bv[256];
    __shared__ int bi[256];
    __shared__ double sh[32];
    __shared__ int jsh;
    const int d = blockIdx.x, tid = threadIdx.x;
    if (!ao_runs(st[d], r)) return;
    double a = 0.0;
    int j = -1;
    for (int e = tid; e < ntile; e += 256) {
        const double v = pval[(size_t)d * ntile + e];
        const int i = pidx[(size_t)d * ntile + e];
        if (ao_before(v, i, a, j)) {
            a = v;
            j = i;
        }
    }
    bv[tid] = a;
    bi[tid] = j;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s && ao_before(bv[tid + s], bi[tid + s], bv[tid], bi[tid])) {
            bv[tid] = bv[tid + s];
            bi[tid] = bi[tid + s];
        }
        __syncthreads();
    }
    if (tid == 0) {
        AoState& s = st[d];
        a = bv[0];
        j = bi[0];
        int sw = 0;
        if (j < 0) {   // no finite exchange value: the design stops as it stands
            s.status |= ACE_ST_AOPT_SINGULAR;
            s.live = 0;
        } else if (a < acutoff || rowlist[(size_t)d * nrows_max + r] < 0) {
            sw = 1;
            s.acrit += a;
            s.switches += 1;
            s.made = 1;
            s.j = j;
            s.wp = 1.0 / (1.0 + gn[(size_t)d * P + j]);
            rowlist[(size_t)d * nrows_max + r] = j;
            cur[(size_t)d * nrows_max + r] = j;
        }
        s.sw = sw;
        jsh = sw ? j : -1;
    }
    __syncthreads();
    j = jsh;
    if (j < 0) return;   // (block-uniform)
    const d2* f = F + (size_t)j * n;
    const d2* u = U + (size_t)d * n;
    double v[2] = {0.0, 0.0};
    for (int k = tid; k < n; k += 256) {   // u^H x_j = sum_k conj(u_k) conj(f_k)
        const d2 a2 = u[k], b = f[k];
        v[0] += a2.x * b.x - a2.y * b.y;
        v[1] -= a2.x * b.y + a2.y * b.x;
    }
    block_sum(v, sh);
    if (tid == 0) st[d].c = make_double2(v[0], v[1]);
}

// ---------------------------------------------------------------- passes
__global__ __launch_bounds__(256) void ao_pass_begin_kernel(int designs, AoState* __restrict__ st) {
    for (int d = threadIdx.x; d < designs; d += 256)
        if (st[d].live) {
            st[d].iters += 1;
            st[d].made = 0;
            st[d].sw = 0;
        }
}

__global__ __launch_bounds__(256) void ao_pass_end_kernel(int designs, int maxiter, AoState* __restrict__ st,
                                                          int32_t* __restrict__ nlive) {
    __shared__ int cnt[256];
    int mine = 0;
    for (int d = threadIdx.x; d < designs; d += 256) {
        if (st[d].live && !(st[d].made && st[d].iters < maxiter)) st[d].live = 0;
        mine += st[d].live;
    }
    cnt[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int v = 0; v < 256; ++v) tot += cnt[v];
        *nlive = tot;
    }
}

__global__ __launch_bounds__(256) void ao_finish_kernel(int designs, const AoState* __restrict__ st,
                                                        double* __restrict__ acrit, int32_t* __restrict__ iters,
                                                        int32_t* __restrict__ switches, uint32_t* __restrict__ status) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= designs) return;
    acrit[2 * d] = st[d].acrit0;
    acrit[2 * d + 1] = st[d].acrit;
    iters[d] = st[d].iters;
    switches[d] = st[d].switches;
    if (status) status[d] = st[d].status;
}

bool ao_limits(int designs, int P, int n, int nrows_max) {
    return designs >= 1 && n >= 1 && n <= AO_NMAX && P >= 1 && P <= AO_PMAX && nrows_max >= 1 && nrows_max <= AO_RMAX;
}

int ao_check_args(const ace_aopt_cfg* cfg, int designs, int P, int n, int nrows_max, const double* F,
                  const int32_t* nrows, const int32_t* init, const int32_t* rowlist, const double* acrit,
                  const int32_t* iters, const int32_t* switches) {
    if (!cfg) return fail(ACE_ERR_ARG, "aopt: NULL cfg");
    if (designs < 1) return fail(ACE_ERR_ARG, "aopt: designs %d < 1", designs);
    if (n < 1 || n > AO_NMAX) return fail(n < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "aopt: n %d outside 1..%d", n, AO_NMAX);
    if (P < 1 || P > AO_PMAX) return fail(P < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "aopt: P %d outside 1..%d", P, AO_PMAX);
    if (nrows_max < 1 || nrows_max > AO_RMAX)
        return fail(nrows_max < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "aopt: nrows_max %d outside 1..%d", nrows_max, AO_RMAX);
    if (cfg->maxiter < 1) return fail(ACE_ERR_ARG, "aopt: maxiter %d < 1", cfg->maxiter);
    if (!(cfg->kdiag > 0.0) || !std::isfinite(cfg->kdiag)) return fail(ACE_ERR_ARG, "aopt: kdiag %g is not positive and finite", cfg->kdiag);
    if (!std::isfinite(cfg->acutoff)) return fail(ACE_ERR_ARG, "aopt: acutoff %g is not finite", cfg->acutoff);
    if (!F || !nrows || !init || !rowlist || !acrit || !iters || !switches)
        return fail(ACE_ERR_ARG, "aopt: NULL %s", !F ? "F" : !nrows ? "nrows" : !init ? "init" : !rowlist ? "rowlist"
                                                  : !acrit ? "acrit" : !iters ? "iters" : "switches");
    return ACE_OK;
}

size_t ao_ws_bytes(int designs, int P, int n, int nrows_max) {
    Carver cv{nullptr};
    AoBufs b;
    ao_carve(cv, designs, P, n, nrows_max, &b);
    return cv.off + 256;   // (the base is rounded up to 256 B)
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" void ace_aopt_cfg_default(ace_aopt_cfg* cfg) {
    if (!cfg) return;
    cfg->maxiter = 5;
    cfg->reserved = 0;
    cfg->kdiag = 1.0;
    cfg->acutoff = -0x1p-26;   // -sqrt(eps)
}

extern "C" size_t ace_aopt_workspace_size(int designs, int P, int n, int nrows_max) {
    if (!ao_limits(designs, P, n, nrows_max)) return 0;
    return ao_ws_bytes(designs, P, n, nrows_max);
}

extern "C" int ace_aopt_select_batch(const ace_aopt_cfg* cfg, int designs, int P, int n, int nrows_max, const double* F,
                                     const int32_t* nrows, const int32_t* init, int32_t* rowlist, double* acrit,
                                     int32_t* iters, int32_t* switches, uint32_t* status, double* Minv_out,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(ao_check_args(cfg, designs, P, n, nrows_max, F, nrows, init, rowlist, acrit, iters, switches));
    const size_t need = ao_ws_bytes(designs, P, n, nrows_max);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "aopt: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    Carver cv{(char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255)};
    AoBufs b;
    ao_carve(cv, designs, P, n, nrows_max, &b);
    const d2* Fc = (const d2*)F;
    const int ntile = ao_ntile(P), ngrp = (designs + AO_DG - 1) / AO_DG, nt16 = (n + 15) / 16;
    const dim3 blk(256);

    // start: rows, Minv = (X^H X + kdiag I)^-1, Acrit, g, t
    hipLaunchKernelGGL(ao_prep_kernel, dim3(designs), blk, 0, s, P, nrows_max, nrows, init, b.cur, rowlist, b.st);
    hipLaunchKernelGGL(ao_gram_kernel, dim3(nt16, nt16, designs), blk, 0, s, n, nrows_max, cfg->kdiag, Fc, b.cur, b.st, b.Minv);
    const int trows = nrows_max < n ? nrows_max : n;
    const dim3 gw((n + 255) / 256, n, designs);
    hipLaunchKernelGGL(ao_inv_kernel, dim3(designs), dim3(1024), (size_t)2 * n * sizeof(d2), s, n, b.st, b.Minv);
    hipLaunchKernelGGL(ao_wood_t_kernel, gw, blk, 0, s, n, nrows_max, trows, Fc, b.cur, b.st, b.Minv, b.T);
    hipLaunchKernelGGL(ao_wood_m_kernel, gw, blk, 0, s, n, nrows_max, trows, cfg->kdiag, Fc, b.cur, b.st, b.T, b.Minv);
    hipLaunchKernelGGL(ao_herm_kernel, dim3(nt16, nt16, designs), blk, 0, s, n, cfg->kdiag, b.Minv);
    hipLaunchKernelGGL(ao_trace_kernel, dim3(designs), blk, 0, s, n, b.Minv, b.st);
    hipLaunchKernelGGL(ao_gt_kernel, dim3(ntile, designs), dim3(AO_NT), 0, s, P, n, Fc, b.Minv, b.g, b.t);
    ACE_HIP(hipGetLastError());

    const dim3 gmv((n + AO_WAVES - 1) / AO_WAVES, designs), gsw(ntile, ngrp), gr2((n + 255) / 256, n, designs);
    for (int it = 0; it < cfg->maxiter; ++it) {
        hipLaunchKernelGGL(ao_pass_begin_kernel, dim3(1), blk, 0, s, designs, b.st);
        for (int r = 0; r < nrows_max; ++r) {
            hipLaunchKernelGGL(ao_mv_kernel<0>, gmv, dim3(AO_NT), 0, s, n, nrows_max, r, Fc, b.cur, b.st, b.Minv, b.U, b.UP, b.U);
            hipLaunchKernelGGL(ao_scal1_kernel, dim3(designs), blk, 0, s, n, nrows_max, r, Fc, b.cur, b.U, b.st);
            hipLaunchKernelGGL(ao_mv_kernel<1>, gmv, dim3(AO_NT), 0, s, n, nrows_max, r, Fc, b.cur, b.st, b.Minv, b.U, b.UP, b.V);
            hipLaunchKernelGGL(ao_sweep_kernel<false>, gsw, dim3(AO_NT), 0, s, designs, P, n, r, Fc, b.st, b.U, b.V, b.g, b.t,
                               b.gn, b.tn, b.pval, b.pidx);
            hipLaunchKernelGGL(ao_decide_kernel, dim3(designs), blk, 0, s, P, n, ntile, nrows_max, r, cfg->acutoff, Fc, b.U,
                               b.gn, b.pval, b.pidx, b.cur, rowlist, b.st);
            hipLaunchKernelGGL(ao_mv_kernel<2>, gmv, dim3(AO_NT), 0, s, n, nrows_max, r, Fc, b.cur, b.st, b.Minv, b.U, b.UP, b.UP);
            hipLaunchKernelGGL(ao_scal2_kernel, dim3(designs), blk, 0, s, n, r, b.U, b.UP, b.st);
            hipLaunchKernelGGL(ao_mv_kernel<3>, gmv, dim3(AO_NT), 0, s, n, nrows_max, r, Fc, b.cur, b.st, b.Minv, b.U, b.UP, b.VP);
            hipLaunchKernelGGL(ao_sweep_kernel<true>, gsw, dim3(AO_NT), 0, s, designs, P, n, r, Fc, b.st, b.UP, b.VP, b.g, b.t,
                               b.gn, b.tn, b.pval, b.pidx);
            hipLaunchKernelGGL(ao_rank2_kernel, gr2, blk, 0, s, n, r, b.st, b.U, b.UP, b.Minv);
        }
        hipLaunchKernelGGL(ao_pass_end_kernel, dim3(1), blk, 0, s, designs, cfg->maxiter, b.st, b.nlive);
        ACE_HIP(hipGetLastError());
        int32_t nlive = 0;   // the one read-back of the pass: does any design go on?
        ACE_HIP(read_back(&nlive, b.nlive, sizeof nlive, s));
        if (nlive == 0) break;
    }
    hipLaunchKernelGGL(ao_finish_kernel, dim3((designs + 255) / 256), blk, 0, s, designs, b.st, acrit, iters, switches, status);
    ACE_HIP(hipGetLastError());
    if (Minv_out)
        ACE_HIP(hipMemcpyAsync(Minv_out, b.Minv, (size_t)designs * n * n * sizeof(d2), hipMemcpyDeviceToDevice, s));
    return ACE_OK;
}

extern "C" int ace_aopt_select_host(const ace_aopt_cfg* cfg, int designs, int P, int n, int nrows_max, const double* F,
                                    const int32_t* nrows, const int32_t* init, int32_t* rowlist, double* acrit,
                                    int32_t* iters, int32_t* switches, uint32_t* status, double* Minv_out) {
    g_err.clear();
    ACE_TRY(ao_check_args(cfg, designs, P, n, nrows_max, F, nrows, init, rowlist, acrit, iters, switches));
    for (int d = 0; d < designs; ++d) {
        if (nrows[d] < 1 || nrows[d] > nrows_max)
            return fail(ACE_ERR_ARG, "aopt: nrows[%d] = %d outside 1..nrows_max = %d", d, nrows[d], nrows_max);
        for (int r = 0; r < nrows[d]; ++r) {
            const int32_t v = init[(size_t)d * nrows_max + r];
            if (v < 0 || v >= P) return fail(ACE_ERR_ARG, "aopt: init[%d][%d] = %d outside 0..%d", d, r, v, P - 1);
        }
    }
    const size_t D = designs, wsb = ao_ws_bytes(designs, P, n, nrows_max);
    DevScope dev;
    double *dF, *dac, *dM = nullptr;
    int32_t *dnr, *dinit, *drl, *dit, *dsw;
    uint32_t* dst;
    char* dws;
    ACE_TRY(dev.put(&dF, F, 2 * (size_t)P * n));
    ACE_TRY(dev.put(&dnr, nrows, D));
    ACE_TRY(dev.put(&dinit, init, D * nrows_max));
    ACE_TRY(dev.alloc(&drl, D * nrows_max));
    ACE_TRY(dev.alloc(&dac, 2 * D));
    ACE_TRY(dev.alloc(&dit, D));
    ACE_TRY(dev.alloc(&dsw, D));
    ACE_TRY(dev.alloc(&dst, D));
    if (Minv_out) ACE_TRY(dev.alloc(&dM, 2 * D * n * n));
    ACE_TRY(dev.alloc(&dws, wsb));
    ACE_TRY(ace_aopt_select_batch(cfg, designs, P, n, nrows_max, dF, dnr, dinit, drl, dac, dit, dsw, dst, dM, dws, wsb, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(rowlist, drl, D * nrows_max));
    ACE_TRY(dev.get(acrit, dac, 2 * D));
    ACE_TRY(dev.get(iters, dit, D));
    ACE_TRY(dev.get(switches, dsw, D));
    ACE_TRY(dev.get(status, dst, D));
    return dev.get(Minv_out, dM, 2 * D * n * n);
}
