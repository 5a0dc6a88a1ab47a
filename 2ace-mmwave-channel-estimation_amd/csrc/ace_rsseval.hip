// Held-out RSS evaluation (the testbed's accuracy metric): batched Evaluate_rss
// (reference main/src/evaluate_plot_results/Evaluate_rss.m and its copy under Numerical_Simulation):
//
//   rss_eval   = abs(cb_test * H)
//   Evaluation = mean(abs(rss_eval - rss_test) ./ rss_test)
//
// Per realisation b and test row p:  pred_p = |sum_k CB[p][k] X[b][k]|  (no conjugate on CB),
// rel_p = |pred_p - rss_p| / rss_p, and the metrics are mean, root mean square and maximum of rel_p over
// the usable rows, with their count.
//
// One fused kernel.  The product CB X^T runs on the f64 matrix cores (v_mfma_f64_16x16x4_f64) in the 3M
// form (mma3m / comb3m and the lane maps of ace_mfma.hpp): A = X (rows: realisations), B = CB^T (columns:
// test rows), so D lane l, reg r is realisation (l >> 4) + 4 r, test row l & 15.
//
// Tiling.  A work-group owns RS_BJ = 16 realisations and walks ALL the test rows in tiles of RS_BC = 128
// (8 waves side by side along the test rows, one 16 x 16 block of three accumulators each), RS_BK = 16
// complex of K per step, operands double-buffered through LDS.  The loop is software-pipelined over four
// stages (global -> registers, registers -> LDS, LDS -> fragments, MFMA): a step's MFMAs run on fragments
// read in the previous step, and a global load has two full steps before its data is needed; the step
// sequence runs across the tile boundaries, so the pipeline fills once per launch, not once per tile.
// The [batch][Pt] product never goes to memory (unless pred is asked for): at
// the end of a tile each lane takes the modulus of its four outputs, forms rel against rss and adds it to
// its own running (sum, sum of squares, max, count) of that realisation.
//
// Reduction (deterministic, batch-invariant, no floating-point atomics, no second pass).  Because a
// work-group sees every test row of its realisations, nothing is combined across work-groups.  For one
// realisation the order is fixed by p alone: lane column c = p & 15 of wave w = (p >> 4) & 7 accumulates
// its rows p = 128 t + 16 w + c in increasing t; the 16 columns are summed by the xor butterfly bsum16;
// the 8 waves are summed in increasing w.  Neither the batch, nor b (its place in the 16 x 16 block only
// selects which register and which 16-lane row hold it), nor pred enters.  The product itself is
// position-independent: output (b, p) is the MFMA chain over k = 0, 4, 8, ... of row b and column p, and
// the zero padding of K, of the rows past Pt and of the realisations past batch only adds exact zeros.
//
// LDS: 2 x (16 + 128) rows x 17 complex = 78336 B, requested as dynamic LDS through the kernel's derived
// budget (lds_dyn_budget; a refused request is an error, there is no second path), plus 4.1 KB static for the
// reduction.  Row stride 17: the 16 rows of a fragment read fall on distinct 16-byte slots of the 256-byte
// bank row; the b128 lane groups mix k and k + 1, which costs one two-way collision in 16 at this stride.
//
// Deliberate departures (the reference gives Inf or NaN): a row whose rss is not finite or <= 0 is left
// out of the statistics, counted out of n_used and flagged ACE_ST_RSS_SKIPPED, its pred still written; a
// realisation with a non-finite X entry, or with no usable row, or whose statistics overflow, returns
// 1, 1, 1, n_used = 0 and ACE_ST_EVAL_DEGENERATE.  An all-zero X is not degenerate: pred = 0, rel = 1.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

#pragma clang fp contract(off)

namespace ace {
namespace {

constexpr int RS_BJ = 16;             // realisations per work-group
constexpr int RS_WAVES = 8;           // waves, side by side along the test rows
constexpr int RS_BC = 16 * RS_WAVES;  // test rows per tile
constexpr int RS_BK = 16;             // complex K per step
constexpr int RS_ST = 17;             // LDS row stride (complex)
constexpr int RS_NT = 64 * RS_WAVES;
constexpr int RS_RING = 4;            // stages in flight from global memory
constexpr int RS_PL = RS_BC * RS_BK / RS_NT;   // CB entries staged per thread per step
static_assert(RS_BJ * RS_BK <= RS_NT && RS_BC * RS_BK % RS_NT == 0 && RS_BK % 4 == 0 && RS_ST >= RS_BK, "staging");

__global__ __launch_bounds__(RS_NT) void rsseval_kernel(int batch, int n, int Pt, const d2* __restrict__ X,
                                                        const d2* __restrict__ CB, const double* __restrict__ rss,
                                                        int rss_shared, double* __restrict__ metrics,
                                                        double* __restrict__ pred, uint32_t* __restrict__ status) {
    extern __shared__ __align__(16) unsigned char rs_lds[];   // Xs[2][RS_BJ * RS_ST], Cs[2][RS_BC * RS_ST] (rs_lds_bytes)
    d2* const Xs = (d2*)rs_lds;
    d2* const Cs = Xs + 2 * RS_BJ * RS_ST;
    __shared__ double red[RS_BJ][RS_WAVES][4];
    __shared__ int sbad[RS_BJ], sskip[RS_BJ];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int j0 = blockIdx.x * RS_BJ;
    const int ksteps = (n + RS_BK - 1) / RS_BK;
    const int tiles = (Pt + RS_BC - 1) / RS_BC;
    const int steps = tiles * ksteps;

    if (t < RS_BJ) {
        sbad[t] = 0;
        sskip[t] = 0;
    }

    // staging maps: X tile 16 x 16 (threads 0..255), CB tile 128 x 16 (four entries per thread); 16 consecutive
    // threads read the 256 contiguous bytes of one row.  Stage s = (tile, K step) in flat order.
    const int xr = t / RS_BK, xc = t % RS_BK;
    d2 xring[RS_RING], cring[RS_RING][RS_PL];   // global -> register ring, indexed by constants after unrolling
    bool xbad = false;
    auto gload = [&](int s, int slot) {
        const int tl = s / ksteps, kb = (s - tl * ksteps) * RS_BK;
        if (t < RS_BJ * RS_BK) {
            xring[slot] = make_double2(0.0, 0.0);
            if (j0 + xr < batch && kb + xc < n) xring[slot] = X[(size_t)(j0 + xr) * n + kb + xc];
        }
#pragma unroll
        for (int u = 0; u < RS_PL; ++u) {
            const int q = t + RS_NT * u, cr = q / RS_BK, cc = q % RS_BK;
            const int p = tl * RS_BC + cr;
            cring[slot][u] = make_double2(0.0, 0.0);
            if (p < Pt && kb + cc < n) cring[slot][u] = CB[(size_t)p * n + kb + cc];
        }
    };
    auto lstore = [&](int s, int slot) {   // (the finiteness test waits for the load: here, where the store does too)
        if (t < RS_BJ * RS_BK) {
            xbad |= !isfinite(xring[slot].x) || !isfinite(xring[slot].y);
            Xs[(s & 1) * RS_BJ * RS_ST + xr * RS_ST + xc] = xring[slot];
        }
#pragma unroll
        for (int u = 0; u < RS_PL; ++u) {
            const int q = t + RS_NT * u;
            Cs[(s & 1) * RS_BC * RS_ST + (q / RS_BK) * RS_ST + q % RS_BK] = cring[slot][u];
        }
    };

    // this lane's outputs: realisations j0 + (lane >> 4) + 4 r, test row 128 tile + 16 w + (lane & 15)
    const int col = 16 * w + (lane & 15);
    d2 fv[2][RS_BK / 4], fl[2][RS_BK / 4];   // MFMA fragments of two consecutive stages
    auto fread = [&](int s, int set) {
#pragma unroll
        for (int kk = 0; kk < RS_BK / 4; ++kk) {
            const int k = kk * 4 + (lane >> 4);
            fv[set][kk] = Xs[(s & 1) * RS_BJ * RS_ST + (lane & 15) * RS_ST + k];
            fl[set][kk] = Cs[(s & 1) * RS_BC * RS_ST + col * RS_ST + k];
        }
    };
    double ssum[4] = {0.0, 0.0, 0.0, 0.0}, ssq[4] = {0.0, 0.0, 0.0, 0.0}, smax[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[4] = {0, 0, 0, 0};
    bool skipped[4] = {false, false, false, false};
    double rv[4] = {0.0, 0.0, 0.0, 0.0};   // rss of the current tile's outputs, loaded ahead of its K loop
    auto rload = [&](int tl) {
        const int p = tl * RS_BC + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = j0 + (lane >> 4) + 4 * r;
            rv[r] = 0.0;
            if (p < Pt && j < batch) rv[r] = rss[(rss_shared ? (size_t)0 : (size_t)j * Pt) + p];
        }
    };

    // Pipeline, per stage s: G(s) global -> ring, W(s) ring -> LDS buffer s & 1, R(s) LDS -> fragments,
    // M(s) MFMAs.  Step s runs, after one barrier, W(s + 2), R(s + 1), G(s + 4), M(s): the MFMAs wait for
    // nothing issued in their own step, and a global load has two full steps before its data is stored.
    // The barrier orders R(s) (step s - 1) before W(s + 2), both on buffer s & 1, and W(s + 1) before R(s + 1).
    d4v p1 = d4v{0.0, 0.0, 0.0, 0.0}, p2 = p1, p3 = p1;
#pragma unroll
    for (int i = 0; i < RS_RING; ++i)
        if (i < steps) gload(i, i);
    rload(0);
    lstore(0, 0);
    if (steps > 1) lstore(1, 1);
    __syncthreads();
    fread(0, 0);

    int ks = 0, tile = 0;
    for (int s0 = 0; s0 < steps; s0 += RS_RING) {
#pragma unroll
        for (int i = 0; i < RS_RING; ++i) {
            const int s = s0 + i;
            if (s < steps) {   // (block-uniform)
                __syncthreads();
                if (s + 2 < steps) lstore(s + 2, (i + 2) % RS_RING);
                if (s + 1 < steps) fread(s + 1, (i + 1) & 1);
                if (s + RS_RING < steps) gload(s + RS_RING, i);
#pragma unroll
                for (int kk = 0; kk < RS_BK / 4; ++kk) mma3m(p1, p2, p3, fv[i & 1][kk], fl[i & 1][kk]);
                if (++ks == ksteps) {   // end of a tile: modulus, relative error, running statistics
                    const int p = tile * RS_BC + col;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = j0 + (lane >> 4) + 4 * r;
                        if (p < Pt && j < batch) {
                            const d2 g = comb3m(p1[r], p2[r], p3[r]);
                            const double pr = hypot(g.x, g.y);
                            if (pred) pred[(size_t)j * Pt + p] = pr;
                            const double rs = rv[r];
                            if (isfinite(rs) && rs > 0.0) {
                                const double rel = fabs(pr - rs) / rs;
                                ssum[r] += rel;
                                ssq[r] += rel * rel;
                                smax[r] = fmax(smax[r], rel) + 0.0 * rel;   // (fmax alone would drop a NaN)
                                ++cnt[r];
                            } else {
                                skipped[r] = true;
                            }
                        }
                    }
                    p1 = p2 = p3 = d4v{0.0, 0.0, 0.0, 0.0};
                    ks = 0;
                    ++tile;
                    if (tile < tiles) rload(tile);
                }
            }
        }
    }
    __syncthreads();

    // ---------------- per realisation: 16 columns (butterfly), then the 8 waves in order
    if (xbad) sbad[xr] = 1;   // (every writer stores the same value)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jl = (lane >> 4) + 4 * r;
        const double s1 = bsum16(ssum[r]), s2 = bsum16(ssq[r]), mx = bmax16(smax[r]) + 0.0 * bsum16(smax[r]);
        const double c = bsum16((double)cnt[r]);
        if (skipped[r]) sskip[jl] = 1;
        if ((lane & 15) == 0) {
            red[jl][w][0] = s1;
            red[jl][w][1] = s2;
            red[jl][w][2] = mx;
            red[jl][w][3] = c;
        }
    }
    __syncthreads();
    if (t < RS_BJ && j0 + t < batch) {
        double s1 = 0.0, s2 = 0.0, mx = 0.0, c = 0.0;
        for (int q = 0; q < RS_WAVES; ++q) {
            s1 += red[t][q][0];
            s2 += red[t][q][1];
            mx = fmax(mx, red[t][q][2]) + 0.0 * red[t][q][2];
            c += red[t][q][3];
        }
        double out[4] = {1.0, 1.0, 1.0, 0.0};
        uint32_t st = (sskip[t] ? ACE_ST_RSS_SKIPPED : 0u) | ACE_ST_EVAL_DEGENERATE;
        if (!sbad[t] && c > 0.0) {
            const double mean = s1 / c, rms = sqrt(s2 / c);
            if (isfinite(mean) && isfinite(rms) && isfinite(mx)) {
                out[0] = mean;
                out[1] = rms;
                out[2] = mx;
                out[3] = c;
                st &= ~ACE_ST_EVAL_DEGENERATE;
            }
        }
        const size_t b = (size_t)(j0 + t);
#pragma unroll
        for (int i = 0; i < 4; ++i) metrics[4 * b + i] = out[i];
        if (status) status[b] = st;
    }
}

constexpr size_t rs_lds_bytes() { return 2 * (size_t)(RS_BJ + RS_BC) * RS_ST * sizeof(d2); }

int rs_check_args(int batch, int n, int Pt, const double* X, const double* CB, const double* rss, int rss_shared,
                  const double* metrics) {
    if (batch < 1) return fail(ACE_ERR_ARG, "rss_evaluate: batch %d < 1", batch);
    if (n < 1) return fail(ACE_ERR_ARG, "rss_evaluate: n %d < 1", n);
    if (Pt < 1) return fail(ACE_ERR_ARG, "rss_evaluate: Pt %d < 1", Pt);
    if (!X || !CB || !rss || !metrics)
        return fail(ACE_ERR_ARG, "rss_evaluate: NULL %s", !X ? "X" : !CB ? "CB" : !rss ? "rss" : "metrics");
    if (rss_shared != 0 && rss_shared != 1) return fail(ACE_ERR_ARG, "rss_evaluate: rss_shared %d not 0 or 1", rss_shared);
    if ((long long)((Pt + RS_BC - 1) / RS_BC) * ((n + RS_BK - 1) / RS_BK) > 0x7fffffffLL)
        return fail(ACE_ERR_ARG, "rss_evaluate: n %d x Pt %d too large", n, Pt);
    return ACE_OK;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_rss_evaluate_batch(int batch, int n, int Pt, const double* X, const double* CB, const double* rss,
                                      int rss_shared, double* metrics, double* pred, uint32_t* status, void* stream) {
    g_err.clear();
    ACE_TRY(rs_check_args(batch, n, Pt, X, CB, rss, rss_shared, metrics));
    // 78336 B of dynamic LDS, past the 64 KiB default: the kernel's derived budget decides (no fallback)
    if (!lds_ok(reinterpret_cast<const void*>(&rsseval_kernel), rs_lds_bytes()))
        return fail(ACE_ERR_UNSUPPORTED, "rss_evaluate: rsseval_kernel needs %zu B of dynamic LDS, budget %zu B",
                    rs_lds_bytes(), lds_dyn_budget(reinterpret_cast<const void*>(&rsseval_kernel)));
    hipLaunchKernelGGL(rsseval_kernel, dim3((batch + RS_BJ - 1) / RS_BJ), dim3(RS_NT), rs_lds_bytes(), (hipStream_t)stream, batch, n,
                       Pt, (const d2*)X, (const d2*)CB, rss, rss_shared, metrics, pred, status);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_rss_evaluate_host(int batch, int n, int Pt, const double* X, const double* CB, const double* rss,
                                     int rss_shared, double* metrics, double* pred, uint32_t* status) {
    g_err.clear();
    ACE_TRY(rs_check_args(batch, n, Pt, X, CB, rss, rss_shared, metrics));
    const size_t B = batch, P = Pt;
    DevScope d;
    double *dX, *dCB, *drss, *dmet, *dpred = nullptr;
    uint32_t* dst;
    ACE_TRY(d.put(&dX, X, 2 * B * n));
    ACE_TRY(d.put(&dCB, CB, 2 * P * n));
    ACE_TRY(d.put(&drss, rss, (rss_shared ? 1 : B) * P));
    ACE_TRY(d.alloc(&dmet, 4 * B));
    if (pred) ACE_TRY(d.alloc(&dpred, B * P));
    ACE_TRY(d.alloc(&dst, B));
    ACE_TRY(ace_rss_evaluate_batch(batch, n, Pt, dX, dCB, drss, rss_shared, dmet, dpred, dst, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(metrics, dmet, 4 * B));
    ACE_TRY(d.get(pred, dpred, B * P));
    return d.get(status, dst, B);
}
