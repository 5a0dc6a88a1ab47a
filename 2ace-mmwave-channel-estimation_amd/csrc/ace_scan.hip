// Beam scan (the reference's exhaustive sweep MyBeamSweeping.m:109-125, and the angular map
// Leakage = A_Rx' * H * A_Tx of Sparse_Channel_Formulation.m:149), batched and fused with its selection:
//
//   y[b][p][q] = sum_i sum_j conj(W0[q][i]) x_b[i + d0 j] F1[p][j]        (w' * H * f)
//   P          = |y + noise|^2,   flat index f = p Q0 + q                  (:124-125, zero-based)
//   top_pow / top_idx = the K largest P of the realisation, total = sum of P.
//
// One fused kernel, one work-group (8 waves) per realisation.  Both products run on the f64 matrix cores
// (v_mfma_f64_16x16x4_f64) in the 3M form, with the helpers and the operand and result lane maps of ace_mfma.hpp.
//
// Tiling.  mat(x) sits in LDS for the whole launch, zero-padded to 32 x 32 (xs[i][j]).  The beam pairs are
// walked in tiles of SC_TP = 64 precoders by SC_TQ = 64 combiners, p outer, q inner:
//   stage A (once per p tile): T[p][i] = sum_j F1[p][j] x[i + d0 j], 64 x 32, A = the F1 tile, B = xs^T, one
//            16 x 16 block per wave, written to LDS (Ts).  T never goes to memory.
//   stage B (per q tile):      y[p][q] = sum_i T[p][i] conj(W0[q][i]), A = Ts, B = the W0 tile (conjugated
//            when it is staged: a sign flip, exact); wave w owns combiner block w & 3 and the two precoder
//            blocks of half w >> 2.
// The F1 and W0 tiles share one LDS buffer; the next tile's global loads are issued into registers before
// the current tile's MFMAs and stored after them, so their latency hides behind the matrix cores.  Rows and
// columns past Q0, Q1, d0, d1 are masked at the loads (zero-filled in LDS: they add exact zeros to the
// products) and at the epilogue; nothing is read or written past the end of an array.
//
// Epilogue and reduction (deterministic, batch-invariant, no atomics, no second pass).  A work-group sees
// every beam pair of its realisation, so nothing is combined across work-groups.  Each lane adds the noise,
// forms P and (a) adds it to its own running total, (b) offers (P, f) to its own sorted list of KC >= K
// entries.  The selection is by the order "P larger, or P equal and f smaller": (P, -f) is a strict total
// order on the pairs of a realisation, so the K largest are one definite set in one definite sequence, and
// merging the lanes' lists (K rounds of a wave-wide best-of-heads, then a rank count over the 8 waves'
// K entries) gives that sequence whatever the order of the merge.  The total's order is fixed by the sizes
// alone: lane-local in tile order, the xor butterfly over the wave, the 8 waves in increasing w.  Neither
// the batch, nor b, nor power / total being requested enters.  KC (1, 4 or 16, the smallest >= K) only sizes
// the lists.
//
// LDS: (32 + 64 + 64) rows x 33 complex = 84480 B of dynamic LDS, requested through the kernel's derived
// budget (lds_dyn_budget; a refused request is an error, there is no second path), plus 1.6 KB static for
// the merge.  Row stride 33: the 16 rows of a fragment read fall on distinct 16-byte slots.
//
// Degenerate realisations: a non-finite entry of x, or of the realisation's noise row, gives powers 0,
// indices -1, total 0 and ACE_ST_EVAL_DEGENERATE (its power row is whatever the product gives).  An all-zero
// x is not degenerate.  Non-finite beams are the caller's error and are not checked.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

#pragma clang fp contract(off)

namespace ace {
namespace {

constexpr int SC_WAVES = 8;
constexpr int SC_NT = 64 * SC_WAVES;
constexpr int SC_D = 32;              // largest d0, d1
constexpr int SC_TP = 64;             // precoders (rows of F1) per tile
constexpr int SC_TQ = 64;             // combiners (rows of W0) per tile
constexpr int SC_ST = 33;             // LDS row stride (complex)
constexpr int SC_KMAX = 16;           // largest K
constexpr int SC_QMAX = 4096;         // largest Q0, Q1
constexpr int SC_PL = SC_TP * SC_D / SC_NT;   // tile entries staged per thread
static_assert(SC_TP == SC_TQ && SC_TP * SC_D % SC_NT == 0 && SC_D * SC_D % SC_NT == 0 && SC_ST > SC_D, "staging");
static_assert(SC_WAVES == (SC_TP / 16) * (SC_D / 16) && SC_WAVES == 2 * (SC_TQ / 16), "wave roles");

// the selection's strict total order: (P, f) comes before (Q, g)
__device__ __forceinline__ bool sc_before(double P, int f, double Q, int g) { return P > Q || (P == Q && f < g); }

template <int KC>
__global__ __launch_bounds__(SC_NT) void scan_kernel(int d0, int d1, int Q0, int Q1, const d2* __restrict__ X,
                                                     const d2* __restrict__ W0, const d2* __restrict__ F1,
                                                     const d2* __restrict__ noise, int K, double* __restrict__ top_pow,
                                                     int32_t* __restrict__ top_idx, double* __restrict__ total,
                                                     double* __restrict__ power, uint32_t* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char sc_lds[];   // xs[32][33], Ts[64][33], Bs[64][33] (sc_lds_bytes)
    d2* const xs = (d2*)sc_lds;
    d2* const Ts = xs + SC_D * SC_ST;
    d2* const Bs = Ts + SC_TP * SC_ST;
    __shared__ double wlp[SC_WAVES][SC_KMAX], wsum[SC_WAVES];
    __shared__ int wlf[SC_WAVES][SC_KMAX];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const size_t b = blockIdx.x;
    const int nk0 = (d0 + 3) / 4, nk1 = (d1 + 3) / 4;
    const int np = (Q1 + SC_TP - 1) / SC_TP, nq = (Q0 + SC_TQ - 1) / SC_TQ;
    const int steps = np * (nq + 1);   // per p tile: its F1 tile, then the nq tiles of W0
    int bad = 0;

    // mat(x) -> xs[i][j], zero-padded; 32 consecutive threads read 32 consecutive entries of a column
#pragma unroll
    for (int u = 0; u < SC_D * SC_D / SC_NT; ++u) {
        const int e = t + SC_NT * u, i = e % SC_D, j = e / SC_D;
        d2 v = make_double2(0.0, 0.0);
        if (i < d0 && j < d1) v = X[b * d0 * d1 + i + (size_t)d0 * j];
        bad |= !isfinite(v.x) || !isfinite(v.y);
        xs[i * SC_ST + j] = v;
    }

    // tile staging: thread t carries entries (row (t >> 5) + 16 u, column t & 31) of the 64 x 32 tile
    d2 ring[SC_PL];
    auto gload = [&](int s) {
        const int pt = s / (nq + 1), r = s - pt * (nq + 1);
        const d2* const src = r ? W0 : F1;
        const int Q = r ? Q0 : Q1, d = r ? d0 : d1, row0 = (r ? r - 1 : pt) * SC_TP;
        const int c = t & 31;
#pragma unroll
        for (int u = 0; u < SC_PL; ++u) {
            const int row = row0 + (t >> 5) + 16 * u;
            ring[u] = make_double2(0.0, 0.0);
            if (row < Q && c < d) ring[u] = src[(size_t)row * d + c];
            if (r) ring[u].y = -ring[u].y;   // W0 is applied conjugated
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int u = 0; u < SC_PL; ++u) Bs[((t >> 5) + 16 * u) * SC_ST + (t & 31)] = ring[u];
    };

    // this lane's sorted list (descending in the selection's order; (-1, -1): empty) and running total
    double lp[KC];
    int lf[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        lp[i] = -1.0;
        lf[i] = -1;
    }
    double tot = 0.0;

    const int frow = (lane & 15) * SC_ST + (lane >> 4);   // fragment read: row l & 15, k = 4 kk + (l >> 4)
    gload(0);
    for (int s = 0; s < steps; ++s) {
        const int pt = s / (nq + 1), r = s - pt * (nq + 1);
        __syncthreads();   // the previous step's reads of Bs (and, before an F1 tile, of Ts) are done
        lstore();
        __syncthreads();
        if (s + 1 < steps) gload(s + 1);
        if (r == 0) {
            // ---- stage A: T = F1 tile . mat(x)^T; wave w -> precoder block w >> 1, antenna block w & 1
            const int pb = w >> 1, ib = w & 1;
            if (16 * ib < d0) {   // (wave-uniform; the K loop of stage B stops at 4 nk0 <= 16 (ib + 1))
                d4v p1 = d4v{0.0, 0.0, 0.0, 0.0}, p2 = p1, p3 = p1;
#pragma unroll
                for (int kk = 0; kk < SC_D / 4; ++kk)
                    if (kk < nk1)
                        mma3m(p1, p2, p3, Bs[16 * pb * SC_ST + frow + 4 * kk], xs[16 * ib * SC_ST + frow + 4 * kk]);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    Ts[(16 * pb + (lane >> 4) + 4 * q) * SC_ST + 16 * ib + (lane & 15)] = comb3m(p1[q], p2[q], p3[q]);
            }
        } else {
            // ---- stage B: y = T . conj(W0 tile)^T; wave w -> combiner block w & 3, precoder blocks 2 (w >> 2) + {0, 1}
            const int q = (r - 1) * SC_TQ + 16 * (w & 3) + (lane & 15);
            if ((r - 1) * SC_TQ + 16 * (w & 3) < Q0) {   // (wave-uniform)
                d2 wf[SC_D / 4];
#pragma unroll
                for (int kk = 0; kk < SC_D / 4; ++kk)
                    if (kk < nk0) wf[kk] = Bs[16 * (w & 3) * SC_ST + frow + 4 * kk];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int pb = 2 * (w >> 2) + h, prow = pt * SC_TP + 16 * pb + (lane >> 4);
                    if (pt * SC_TP + 16 * pb < Q1) {   // (wave-uniform)
                        d2 nz[4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) {   // the block's noise, loaded ahead of its MFMAs
                            const int p = prow + 4 * g;
                            nz[g] = make_double2(0.0, 0.0);
                            if (noise && p < Q1 && q < Q0) nz[g] = noise[b * Q1 * Q0 + (size_t)p * Q0 + q];
                        }
                        d4v p1 = d4v{0.0, 0.0, 0.0, 0.0}, p2 = p1, p3 = p1;
#pragma unroll
                        for (int kk = 0; kk < SC_D / 4; ++kk)
                            if (kk < nk0) mma3m(p1, p2, p3, Ts[16 * pb * SC_ST + frow + 4 * kk], wf[kk]);
                        double cp[4];
                        int cf[4];
                        bool offer = false;
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int p = prow + 4 * g;
                            cp[g] = -2.0;   // (comes before nothing: not offered)
                            cf[g] = p * Q0 + q;
                            if (p < Q1 && q < Q0) {
                                bad |= !isfinite(nz[g].x) || !isfinite(nz[g].y);
                                const d2 y = comb3m(p1[g], p2[g], p3[g]);
                                const double yr = y.x + nz[g].x, yi = y.y + nz[g].y;
                                const double P = yr * yr + yi * yi;
                                if (power) power[b * Q1 * Q0 + (size_t)cf[g]] = P;
                                tot += P;
                                cp[g] = P;
                                offer |= sc_before(P, cf[g], lp[KC - 1], lf[KC - 1]);
                            }
                        }
                        if (__any(offer)) {   // (rare once the lists have filled)
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                double vp = cp[g];
                                int vf = cf[g];
#pragma unroll
                                for (int i = 0; i < KC; ++i)
                                    if (sc_before(vp, vf, lp[i], lf[i])) {
                                        const double tp = lp[i];
                                        const int tf = lf[i];
                                        lp[i] = vp;
                                        lf[i] = vf;
                                        vp = tp;
                                        vf = tf;
                                    }
                            }
                        }
                    }
                }
            }
        }
    }

    // ---------------- per wave: the total (xor butterfly) and K rounds of best-of-heads over the lanes' lists
    bad = __syncthreads_or(bad);
    tot = wave_sum(tot);
    if (lane == 0) wsum[w] = tot;
    for (int k = 0; k < K; ++k) {
        double bp = lp[0];
        int bf = lf[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double op = __shfl_xor(bp, o, 64);
            const int of = __shfl_xor(bf, o, 64);
            if (sc_before(op, of, bp, bf)) {
                bp = op;
                bf = of;
            }
        }
        if (lane == 0) {
            wlp[w][k] = bp;
            wlf[w][k] = bf;
        }
        if (lf[0] == bf && lp[0] == bp) {   // the lane that held it moves its list up
#pragma unroll
            for (int i = 0; i + 1 < KC; ++i) {
                lp[i] = lp[i + 1];
                lf[i] = lf[i + 1];
            }
            lp[KC - 1] = -1.0;
            lf[KC - 1] = -1;
        }
    }
    __syncthreads();

    // ---------------- the 8 waves' K entries: an entry's place is the number of entries before it in the order
    if (bad) {   // (block-uniform)
        if (t < K) {
            top_pow[b * K + t] = 0.0;
            top_idx[b * K + t] = -1;
        }
    } else if (t < SC_WAVES * SC_KMAX && (t & (SC_KMAX - 1)) < K) {
        const double P = wlp[t >> 4][t & 15];
        const int f = wlf[t >> 4][t & 15];
        int rank = 0;
        for (int v = 0; v < SC_WAVES; ++v)
            for (int k = 0; k < K; ++k) rank += sc_before(wlp[v][k], wlf[v][k], P, f);
        if (rank < K && f >= 0) {
            top_pow[b * K + rank] = P;
            top_idx[b * K + rank] = f;
        }
    }
    if (t == 0) {
        double s = 0.0;
        for (int v = 0; v < SC_WAVES; ++v) s += wsum[v];
        if (total) total[b] = bad ? 0.0 : s;
        if (status) status[b] = bad ? ACE_ST_EVAL_DEGENERATE : 0u;
    }
}

constexpr size_t sc_lds_bytes() { return (size_t)(SC_D + SC_TP + SC_TQ) * SC_ST * sizeof(d2); }

int sc_check_args(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0, const double* F1, int K,
                  const double* top_pow, const int32_t* top_idx) {
    if (batch < 1) return fail(ACE_ERR_ARG, "beam_scan: batch %d < 1", batch);
    if (d0 < 1 || d0 > SC_D) return fail(ACE_ERR_ARG, "beam_scan: d0 %d outside 1..%d", d0, SC_D);
    if (d1 < 1 || d1 > SC_D) return fail(ACE_ERR_ARG, "beam_scan: d1 %d outside 1..%d", d1, SC_D);
    if (Q0 < 1 || Q0 > SC_QMAX) return fail(ACE_ERR_ARG, "beam_scan: Q0 %d outside 1..%d", Q0, SC_QMAX);
    if (Q1 < 1 || Q1 > SC_QMAX) return fail(ACE_ERR_ARG, "beam_scan: Q1 %d outside 1..%d", Q1, SC_QMAX);
    if (K < 1 || K > SC_KMAX || (long long)K > (long long)Q0 * Q1)
        return fail(ACE_ERR_ARG, "beam_scan: K %d outside 1..min(%d, Q0*Q1 = %lld)", K, SC_KMAX, (long long)Q0 * Q1);
    if (!X || !W0 || !F1 || !top_pow || !top_idx)
        return fail(ACE_ERR_ARG, "beam_scan: NULL %s", !X ? "X" : !W0 ? "W0" : !F1 ? "F1" : !top_pow ? "top_pow" : "top_idx");
    return ACE_OK;
}

template <int KC>
int sc_launch(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0, const double* F1,
              const double* noise, int K, double* top_pow, int32_t* top_idx, double* total, double* power,
              uint32_t* status, hipStream_t st) {
    // 84480 B of dynamic LDS, past the 64 KiB default: the kernel's derived budget decides (no fallback)
    const void* const kern = reinterpret_cast<const void*>(&scan_kernel<KC>);
    if (!lds_ok(kern, sc_lds_bytes()))
        return fail(ACE_ERR_UNSUPPORTED, "beam_scan: scan_kernel needs %zu B of dynamic LDS, budget %zu B", sc_lds_bytes(),
                    lds_dyn_budget(kern));
    hipLaunchKernelGGL(scan_kernel<KC>, dim3(batch), dim3(SC_NT), sc_lds_bytes(), st, d0, d1, Q0, Q1, (const d2*)X,
                       (const d2*)W0, (const d2*)F1, (const d2*)noise, K, top_pow, top_idx, total, power, status);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

}  // namespace

size_t scan_request_bytes() { return sc_lds_bytes(); }

}  // namespace ace

using namespace ace;

extern "C" int ace_beam_scan_batch(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0,
                                   const double* F1, const double* noise, int K, double* top_pow, int32_t* top_idx,
                                   double* total, double* power, uint32_t* status, void* stream) {
    g_err.clear();
    ACE_TRY(sc_check_args(batch, d0, d1, Q0, Q1, X, W0, F1, K, top_pow, top_idx));
    const hipStream_t st = (hipStream_t)stream;
    if (K == 1) return sc_launch<1>(batch, d0, d1, Q0, Q1, X, W0, F1, noise, K, top_pow, top_idx, total, power, status, st);
    if (K <= 4) return sc_launch<4>(batch, d0, d1, Q0, Q1, X, W0, F1, noise, K, top_pow, top_idx, total, power, status, st);
    return sc_launch<SC_KMAX>(batch, d0, d1, Q0, Q1, X, W0, F1, noise, K, top_pow, top_idx, total, power, status, st);
}

extern "C" int ace_beam_scan_host(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0,
                                  const double* F1, const double* noise, int K, double* top_pow, int32_t* top_idx,
                                  double* total, double* power, uint32_t* status) {
    g_err.clear();
    ACE_TRY(sc_check_args(batch, d0, d1, Q0, Q1, X, W0, F1, K, top_pow, top_idx));
    const size_t B = batch, QQ = (size_t)Q0 * Q1;
    DevScope d;
    double *dX, *dW0, *dF1, *dnoise = nullptr, *dpow, *dtotal, *dpower = nullptr;
    int32_t* didx;
    uint32_t* dst;
    ACE_TRY(d.put(&dX, X, 2 * B * d0 * d1));
    ACE_TRY(d.put(&dW0, W0, 2 * (size_t)Q0 * d0));
    ACE_TRY(d.put(&dF1, F1, 2 * (size_t)Q1 * d1));
    if (noise) ACE_TRY(d.put(&dnoise, noise, 2 * B * QQ));
    ACE_TRY(d.alloc(&dpow, B * K));
    ACE_TRY(d.alloc(&didx, B * K));
    ACE_TRY(d.alloc(&dtotal, B));
    if (power) ACE_TRY(d.alloc(&dpower, B * QQ));
    ACE_TRY(d.alloc(&dst, B));
    ACE_TRY(ace_beam_scan_batch(batch, d0, d1, Q0, Q1, dX, dW0, dF1, dnoise, K, dpow, didx, dtotal, dpower, dst, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(top_pow, dpow, B * K));
    ACE_TRY(d.get(top_idx, didx, B * K));
    ACE_TRY(d.get(total, dtotal, B));
    ACE_TRY(d.get(power, dpower, B * QQ));
    return d.get(status, dst, B);
}
