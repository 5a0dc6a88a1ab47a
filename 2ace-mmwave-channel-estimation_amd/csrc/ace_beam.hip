// Downstream beamformer: batched svd_beamformer /
// svd_beamformer_compensation (reference main/codebook_library.py:57-138), the consumer
// of recovered channels in codebook_generator (:192-213).
//
// Per realisation: Vh of zgesdd(H) and of zgesdd(H^T) (JOBZ='A', LAPACK's phase and sign
// convention, because the beam codes quantise those phases), 2-bit phase quantisation,
// the all-pairs received-power search |wt_i^T H wr_j|^2 with first-argmax, and the code
// strings of the winning pair.  One wavefront per realisation, everything in LDS (the SVD
// routines live in ace_svd.hpp, shared with the channel evaluator ace_eval.hip):
//
//   zgebd2     Householder bidiagonalisation (zlarfg conventions), lane = column / row
//   dbdsqr     implicit-shift / zero-shift QR on the real bidiagonal; the scalar recurrence
//              runs redundantly in every lane (uniform control flow, no broadcasts), each
//              lane applies the rotations to its own column of VT as they are generated
//   zunmbr     Vh = VT * P^H, reflectors applied right-to-left, lane = row
//   search     T = H wr (exact +-1/+-j multipliers), M = wt^T T, argmax over lanes
//
// For n <= 25 this is zgesdd's path (dbdsdc -> dlasdq -> dbdsqr).  For 26..32 numpy's
// zgesdd uses divide and conquer (dlasd0: two dlasdq leaves and one dlasd1 merge), whose real
// singular vectors equal dbdsqr's up to sign; the merge's sign convention is applied after
// dbdsqr (gesdd_vh).  The status bit ACE_ST_BF_DC marks those realisations: a vector the merge
// deflated (the null space of a rank-deficient H) can still differ from numpy's.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_svd.hpp"

// No a*b+c -> fma contraction in this file: LAPACK (numpy's scipy-openblas build) evaluates
// dbdsqr's recurrences unfused, and with a converged (perfect) shift the bottom rotation of a
// chase is a cancellation whose rounding decides the sign of a singular vector -- i.e. a
// code bit.  Fused rounding flips it on ~1% of 16x16 matrices.
#pragma clang fp contract(off)

namespace ace {
namespace {

// around(angle(z) / (pi/2)) in -2..2 (numpy's round-half-even == rint)
__device__ __forceinline__ signed char quant(d2 z) { return (signed char)rint(atan2(z.y, z.x) / kHalfPi); }

// argmax order: NaN first (numpy), then larger, ties -> smaller index
__device__ __forceinline__ bool bf_better(double a, int ia, double b, int ib) {
    const bool na = isnan(a), nb = isnan(b);
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// 2-bit code of exp(1j * -(q*pi/2)) * exp(-1j*off) (codebook_library.py:80-88, :122-127)
__device__ __forceinline__ unsigned char code_of(int q, bool has_off, double off) {
    const double th = -((double)q * kHalfPi);
    double re = cos(th), im = sin(th);
    if (has_off) {
        const double br = cos(off), bi = -sin(off);
        const double pr = re * br - im * bi, pi = re * bi + im * br;
        re = pr;
        im = pi;
    }
    double c = rint(atan2(im, re) / kHalfPi);
    if (c < 0) c += 4.0;
    if (c == 4.0) c = 0.0;
    return (unsigned char)c;
}

// RECT = false: tx == rx (the square path only, which keeps the kernel at four waves per SIMD)
template <bool RECT>
__global__ __launch_bounds__(64) void beamformer_kernel(int tx, int rx, const d2* __restrict__ H,
                                                        const double* __restrict__ offset,
                                                        unsigned char* __restrict__ wr_code,
                                                        unsigned char* __restrict__ wt_code, int32_t* __restrict__ beam_idx,
                                                        double* __restrict__ rss_out, uint32_t* __restrict__ status,
                                                        d2* __restrict__ vh_r, d2* __restrict__ vh_t) {
    extern __shared__ __align__(16) unsigned char bf_lds[];
    const int lane = threadIdx.x;
    const int N = max(tx, rx), ld = N + 1;
    const size_t b = blockIdx.x;
    const int nh = tx * rx;
    BfShared sh;
    sh.A = (d2*)bf_lds;
    sh.X = sh.A + N * ld;
    sh.Q = sh.X + N * ld;
    sh.taup = sh.Q + (tx != rx ? N * ld : 0);
    sh.d = (double*)(sh.taup + BF_NMAX);
    sh.e = sh.d + BF_NMAX;
    sh.qr = (signed char*)(sh.e + BF_NMAX);
    sh.qt = sh.qr + rx * rx;
    const d2* Hb = H + b * nh;

    // non-finite input: numpy's zgesdd fails (LinAlgError "SVD did not converge")
    bool bad = false;
    for (int k = lane; k < nh; k += 64) {
        const d2 h = Hb[k];
        bad |= !isfinite(h.x) || !isfinite(h.y);
    }
    uint32_t st = (min(tx, rx) > BF_SMLSIZ) ? ACE_ST_BF_DC : 0u;
    if (__any(bad)) {
        if (lane == 0) {
            status[b] = st | ACE_ST_BF_NONFINITE;
            beam_idx[2 * b] = -1;
            beam_idx[2 * b + 1] = -1;
            rss_out[b] = __builtin_nan("");
        }
        for (int k = lane; k < rx; k += 64) wr_code[b * rx + k] = 0;
        for (int k = lane; k < tx; k += 64) wt_code[b * tx + k] = 0;
        return;
    }
    bool ok = true;
    for (int pass = 0; pass < 2; ++pass) {
        // pass 0: zgesdd(H) [tx][rx] -> Vh [rx][rx] -> wr; pass 1: zgesdd(H^T) [rx][tx] -> [tx][tx] -> wt
        // (codebook_library.py:59-60)
        const int m = pass == 0 ? tx : rx, n = pass == 0 ? rx : tx;
        for (int k = lane; k < nh; k += 64) {
            const int r = k / rx, c = k - r * rx;   // H[r][c]
            if (pass == 0) sh.A[r * ld + c] = Hb[k];
            else sh.A[c * ld + r] = Hb[k];
        }
        wsync();
        ok &= gesdd_vh<RECT>(sh, m, n, ld, lane);
        signed char* q = pass == 0 ? sh.qr : sh.qt;
        d2* vh_out = pass == 0 ? vh_r : vh_t;
        for (int k = lane; k < n * n; k += 64) {
            const int r = k / n, c = k - r * n;
            const d2 v = sh.X[r * ld + c];
            q[k] = quant(v);
            if (vh_out) vh_out[b * n * n + k] = v;
        }
        wsync();
    }
    if (!ok) st |= ACE_ST_BF_NOCONV;
    // ---------------- received-power search (codebook_library.py:67-77)
    // wr_quant[b', j] = j^(-qr[j][b']) (b', j < rx), wt_quant[a, i] = j^(-qt[i][a]) (a, i < tx)
    d2* Hs = sh.A;
    d2* T = sh.X;
    for (int k = lane; k < nh; k += 64) {
        const int r = k / rx, c = k - r * rx;
        Hs[r * ld + c] = Hb[k];
    }
    wsync();
    for (int k = lane; k < nh; k += 64) {  // T[a][j] = sum_b H[a][b] wr[b][j]
        const int a = k / rx, j = k - a * rx;
        d2 acc = make_double2(0.0, 0.0);
        for (int bb = 0; bb < rx; ++bb) acc = cadd(acc, rotk(Hs[a * ld + bb], -sh.qr[j * rx + bb]));
        T[a * ld + j] = acc;
    }
    wsync();
    double best = -__builtin_inf();
    int bidx = 0x7fffffff;
    for (int k = lane; k < nh; k += 64) {  // M[i][j] = sum_a wt[a][i] T[a][j], i-major (i < tx, j < rx)
        const int i = k / rx, j = k - i * rx;
        d2 acc = make_double2(0.0, 0.0);
        for (int a = 0; a < tx; ++a) acc = cadd(acc, rotk(T[a * ld + j], -sh.qt[i * tx + a]));
        const double amp = hypot(acc.x, acc.y);
        const double rss = 10.0 * log10(amp * amp * 1000.0);
        if (bf_better(rss, k, best, bidx)) { best = rss; bidx = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (bf_better(ob, oi, best, bidx)) { best = ob; bidx = oi; }
    }
    const int tx_idx = bidx / rx, rx_idx = bidx - tx_idx * rx;
    // offset [batch][N]: entry k compensates element k of both codes (numpy broadcasting of the reference's
    // `* np.exp(-1j * offset)`, :122-127; tx != rx admits only a constant offset there)
    const bool has_off = offset != nullptr;
    for (int k = lane; k < rx; k += 64)
        wr_code[b * rx + k] = code_of(sh.qr[rx_idx * rx + k], has_off, has_off ? offset[b * N + k] : 0.0);
    for (int k = lane; k < tx; k += 64)
        wt_code[b * tx + k] = code_of(sh.qt[tx_idx * tx + k], has_off, has_off ? offset[b * N + k] : 0.0);
    if (lane == 0) {
        beam_idx[2 * b] = tx_idx;
        beam_idx[2 * b + 1] = rx_idx;
        rss_out[b] = best;
        status[b] = st;
    }
}

size_t bf_lds_bytes(int tx, int rx) {
    const size_t N = std::max(tx, rx);
    return (size_t)(tx != rx ? 3 : 2) * N * (N + 1) * sizeof(d2) + BF_NMAX * sizeof(d2) +
           2 * BF_NMAX * sizeof(double) + (size_t)tx * tx + (size_t)rx * rx;
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" int ace_svd_beamformer_batch(int batch, int tx, int rx, const double* H, const double* offset,
                                        uint8_t* wr_code, uint8_t* wt_code, int32_t* beam_idx, double* rss,
                                        uint32_t* status, double* vh_r, double* vh_t, void* stream) {
    g_err.clear();
    if (batch < 0) return fail(ACE_ERR_ARG, "svd_beamformer: batch %d < 0", batch);
    if (tx < 1 || tx > BF_NMAX || rx < 1 || rx > BF_NMAX)
        return fail(ACE_ERR_UNSUPPORTED, "svd_beamformer: %d x %d antennas outside 1..%d", tx, rx, BF_NMAX);
    if (batch == 0) return ACE_OK;
    if (!H || !wr_code || !wt_code || !beam_idx || !rss || !status)
        return fail(ACE_ERR_ARG, "svd_beamformer: null output/input pointer");
    const size_t lds = bf_lds_bytes(tx, rx);
    hipLaunchKernelGGL(tx == rx ? beamformer_kernel<false> : beamformer_kernel<true>, dim3(batch), dim3(64), lds,
                       (hipStream_t)stream, tx, rx, (const d2*)H, offset,
                       wr_code, wt_code, beam_idx, rss, status, (d2*)vh_r, (d2*)vh_t);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_svd_beamformer_host(int batch, int tx, int rx, const double* H, const double* offset,
                                       uint8_t* wr_code, uint8_t* wt_code, int32_t* beam_idx, double* rss,
                                       uint32_t* status, double* vh_r, double* vh_t) {
    g_err.clear();
    if (batch < 0 || tx < 1 || tx > BF_NMAX || rx < 1 || rx > BF_NMAX)
        return ace_svd_beamformer_batch(batch, tx, rx, H, offset, wr_code, wt_code, beam_idx, rss, status, vh_r,
                                        vh_t, nullptr);
    if (batch == 0) return ACE_OK;
    const size_t B = batch, N = std::max(tx, rx), nvr = 2 * B * rx * rx, nvt = 2 * B * tx * tx;   // doubles
    DevScope d;
    double *dH, *doff = nullptr, *drss, *dvr = nullptr, *dvt = nullptr;
    uint8_t *dwr, *dwt;
    int32_t* didx;
    uint32_t* dst;
    ACE_TRY(d.put(&dH, H, 2 * B * tx * rx));
    if (offset) ACE_TRY(d.put(&doff, offset, B * N));
    ACE_TRY(d.alloc(&dwr, B * rx));
    ACE_TRY(d.alloc(&dwt, B * tx));
    ACE_TRY(d.alloc(&didx, 2 * B));
    ACE_TRY(d.alloc(&drss, B));
    ACE_TRY(d.alloc(&dst, B));
    if (vh_r) ACE_TRY(d.alloc(&dvr, nvr));
    if (vh_t) ACE_TRY(d.alloc(&dvt, nvt));
    ACE_TRY(ace_svd_beamformer_batch(batch, tx, rx, dH, doff, dwr, dwt, didx, drss, dst, dvr, dvt, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(wr_code, dwr, B * rx));
    ACE_TRY(d.get(wt_code, dwt, B * tx));
    ACE_TRY(d.get(beam_idx, didx, 2 * B));
    ACE_TRY(d.get(rss, drss, B));
    ACE_TRY(d.get(status, dst, B));
    ACE_TRY(d.get(vh_r, dvr, nvr));
    return d.get(vh_t, dvt, nvt);
}
