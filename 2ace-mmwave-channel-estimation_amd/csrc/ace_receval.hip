// Sparse-recovery evaluation: batched Evaluation_Recovery (reference
// Numerical_Simulation/src/evaluate_plot_results/Evaluation_Recovery.m:73-338), the score the reference gives the
// recoveries on the angular dictionary (PLOMP, PLGAMP, PerfectPhaseCS, NoisyPhaseCS, PRGAMP: Vs_M.m:215-221,
// Vs_SNR.m:192-194, sub_VS_SR_par.m:166-170), and pattern 1's angle estimate of MyBeamSweeping.m:134-154.
//
// Per realisation, from the sparse vector z [Qt*Qr] (index u Qr + v, sparse.dictionary_2d's), the true channel
// vecH (element r + rx t), the true angles and the two sweep picks, the 15 numbers of :322-336:
//
//   0  Num_Quantization_Error   (:149-161; only for L == 1, else 0)
//   1  AoDA_Err                 (:135-146)            8  Rate_BSweep1     (:232, :272, :281)
//   2  MSE_ARM                  (:165-183)            9  Rate_BSweep2     (:233, :273, :282)
//   3  MSE_H                    (:187-191)           10  AoDA_Err_Sweep1  (:246-259)
//   4  Rate_Unconstrained       (:196-201, :277)     11  AoDA_Err_Sweep2
//   5  Rate_PerCSI              (:202-203, :278)     12  gain_ana         (:289-298)
//   6  Rate_Est                 (:212-217, :279)     13  gain_dig         (:299)
//   7  Rate_Est_AoDA            (:226-229, :280)     14  proj_error       (:309-317)
//
// The reference as it stands, restated:
//   * :86 sorts the complex z by modulus; an exact modulus tie goes to the LOWER index here (MATLAB breaks it by
//     phase angle: a deliberate departure, it only matters for exactly tied entries such as the zeros of an OMP
//     output with fewer than L atoms).  :88 puts the L picks in ascending index order.
//   * :127-132: the true AoD are sorted descending and the true quantised angles follow that order; :128 assigns
//     AoA_True(order) = AoA_True(order), a no-op, so the true AoA keep the scenario's order.  The estimated pairs are
//     ordered by estimated AoD descending (stable), the AoA following.
//   * :149-161: the quantisation error exists for L == 1 only and is in global grid index units.
//   * :194 Num_RFchains = 1: every beam goes through Quantize_PS (2 bits, exact powers of j); HybridPrecoding is
//     never reached.
//   * :226-227 read AoD_Estimated(l) with l left over from the loop of :169: the LAST entry after the sort of :131.
//   * :277-282: eye(L) + scalar adds the scalar to every entry, det = 1 + L |g|^2 / sigma^2; the rate is |log2| of it.
//   * :289-317: columns 12-14 are Evaluation_H's gain_ana, gain_dig and proj_err of (H_est, H); Rate_Est is the rate
//     of column 12's gain, Rate_PerCSI that of the quantised top pair of H on H, Rate_Unconstrained that of s1(H).
//   * The save calls of :262-265 and :337 are dropped.  The sweep itself (MyBeamSweeping) is not redone: the caller
//     passes the beam indices ace_beam_scan_batch picked for pattern 1 and pattern 2, and the tables of their angle
//     estimates.  Patterns 1 and 2 quantise the same phases (Quantize_PS normalises, so Directional_Beam_Angular.m:79-85
//     and MyBeamSweeping.m:101-108 give the same F, W); they differ in the estimate and in their noise draws.
//
// H_est = AD z is never formed as a dense product: AD = kron(conj(A_t), A_r), so with Z[u][v] = z[u Qr + v]
//   H_est [rx][tx] = A_r^T [rx][Qr] . Z^T [Qr][Qt] . conj(A_t) [Qt][tx],
// two small complex products on the f64 matrix cores (cmma of ace_mfma.hpp).  z is read from memory once, as the B
// operand of the first product, in tiles of 16 values of u by 4 of v; the modulus, the finiteness test and each
// lane's running top-8 ride on that load.  A tile's 16 columns of T = A_r^T Z^T go through LDS (Ts) to become the A
// operand of the second product; H_est stays in accumulators until the last tile.  mat(z) (256 KiB at Qt = Qr = 128)
// is therefore never held on chip, and the dictionaries are read through L2, which every block shares.
//
// LDS budget (one wavefront per realisation; N = max(tx, rx), ld = N + 1, nh = tx rx), dynamic:
//   SVD workspace  (2, or 3 for tx != rx) N ld c128   the carve of evaluate_kernel (ace_svd.hpp's BfShared)
//   taup, u1, v1, ug, vg                5 * 32 c128
//   d, e                                2 * 32 f64
//   Hs, Gs                              2 N^2 c128    H_est and H
//   Ts                                  NT 16 * 17 c128, NT = ceil(N / 16)
// = 24 320 B at 16 x 16, 78 336 B at 32 x 32 and 95 232 B at 32 x 31 (rectangular), past the 64 KiB default through
// the kernel's derived budget (lds_dyn_budget), plus 576 B static for the codes and the angle lists.
// ace_lds_request("receval" / "receval_rect", N) reports it; tests/test_receval_lds.py checks static + dynamic
// against the CU's 160 KiB.
//
// The SVD part is ace_eval.hip's: gesdd_vh of ace_svd.hpp in numpy's gauge (v = conj(row 0 of Vh of zgesdd(M)),
// u = row 0 of Vh of zgesdd(M^T)) for M = H_est and M = H, and the same entry-by-entry sums for gain_dig and
// proj_err.  The matrix is rx x tx with entry (r, t) = v[r + rx t]: ace_evaluate_batch(H_est, H, rx, tx) in that
// entry's terms.
//
// Degenerate realisations (a non-finite or all-zero z, a non-finite or zero H, an H_est that comes out zero or not
// finite, a metric that overflows) follow the evaluator: MSE_H = MSE_ARM = proj_error = 1, gains and rates 0,
// ACE_ST_EVAL_DEGENERATE; with a degenerate z the angle errors are those of the lowest-index picks 0 .. L - 1, and
// H_est is written as zeros.  Without sweep picks (picks == NULL, or an index outside its table for that row)
// columns 8-11 are NaN and ACE_ST_RECEVAL_NOSWEEP is set.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"
#include "ace_svd.hpp"

#include <climits>
#include <cmath>

#pragma clang fp contract(off)

namespace ace {
namespace {

constexpr int RV_LMAX = 8, RV_QMAX = 4096, RV_MMAX = 4096;
constexpr int RV_TS = 17;            // row stride of Ts
constexpr int PK_NT = 256;           // threads of peak_kernel
constexpr int PK_NANG = 36001;       // -90 : 0.005 : 90
constexpr double kDeg = 0.017453292519943295;   // numpy's deg2rad factor, pi / 180

struct RvArgs {
    int tx, rx, L, Qt, Qr, first_t, first_r, Mt, Mr;
    double noise_power, kappa;
    const d2 *At, *Ar;
    const double *deg_t, *deg_r;
    const d2 *z, *vecH;
    const double *aod, *aoa;
    const int32_t *tidx, *picks;
    const double *cen_t, *cen_r, *pk_t, *pk_r;
    double* metrics;
    d2* Hest;
    uint32_t* status;
};

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ d2 rv_wave_csum(d2 v) { return make_double2(wave_sum(v.x), wave_sum(v.y)); }

// entry k of the unit-modulus steering vector at `deg` degrees: exp(-j kappa sin(deg) k)
__device__ __forceinline__ d2 rv_steer(double kappa, double deg, int k) {
    const double ph = kappa * sin(deg * kDeg) * (double)k;
    return make_double2(cos(ph), -sin(ph));
}

// |log2(1 + L g^2 / sigma^2)|  (:277-282)
__device__ __forceinline__ double rv_rate(double g, int L, double np) { return fabs(log2(1.0 + (double)L * (g * g) / np)); }

// RECT = false: tx == rx (gesdd_vh's square path alone, as in evaluate_kernel); NT * 16 >= max(tx, rx)
template <bool RECT, int NT>
__global__ __launch_bounds__(64) void receval_kernel(const RvArgs a) {
    extern __shared__ __align__(16) unsigned char rv_lds[];
    __shared__ int s_qa[BF_NMAX], s_qb[BF_NMAX], s_pick[RV_LMAX];
    __shared__ double s_eD[RV_LMAX], s_eA[RV_LMAX], s_tD[RV_LMAX], s_tA[RV_LMAX], s_sc[4];
    const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
    const int tx = a.tx, rx = a.rx, L = a.L, Qt = a.Qt, Qr = a.Qr;
    const int m = rx, n = tx;   // the matrix is rx x tx, entry (i, j) = v[i + m j]
    const int N = max(tx, rx), ld = N + 1, nh = tx * rx;
    const size_t b = blockIdx.x;
    BfShared sh;
    sh.A = (d2*)rv_lds;
    sh.X = sh.A + N * ld;
    sh.Q = sh.X + N * ld;
    sh.taup = sh.Q + (RECT ? N * ld : 0);
    d2* u1 = sh.taup + BF_NMAX;   // [m] top left vector of H_est
    d2* v1 = u1 + BF_NMAX;        // [n] top right vector of H_est
    d2* ug = v1 + BF_NMAX;        // [m] ... of H
    d2* vg = ug + BF_NMAX;        // [n]
    sh.d = (double*)(vg + BF_NMAX);
    sh.e = sh.d + BF_NMAX;
    d2* Hs = (d2*)(sh.e + BF_NMAX);   // [nh] H_est
    d2* Gs = Hs + nh;                 // [nh] H
    d2* Ts = Gs + nh;                 // [NT * 16][RV_TS]
    sh.qr = nullptr;
    sh.qt = nullptr;

    // ---------------- the one read of z: T = A_r^T Z^T per tile of 16 u, H_est += T conj(A_t); top-8 per lane
    const d2* zb = a.z + b * (size_t)Qt * Qr;
    d4v Hr[NT][NT], Hi[NT][NT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) Hr[i][j] = Hi[i][j] = d4v{0.0, 0.0, 0.0, 0.0};
    double tm[RV_LMAX];
    int ti[RV_LMAX];
#pragma unroll
    for (int j = 0; j < RV_LMAX; ++j) {
        tm[j] = -1.0;
        ti[j] = INT_MAX;
    }
    bool bad = false;
    for (int u0 = 0; u0 < Qt; u0 += 16) {
        d4v Tr[NT], Ti[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) Tr[i] = Ti[i] = d4v{0.0, 0.0, 0.0, 0.0};
        const int u = u0 + lr;
        for (int v0 = 0; v0 < Qr; v0 += 4) {
            const int v = v0 + lk;
            d2 zv = make_double2(0.0, 0.0);
            if (u < Qt && v < Qr) {
                zv = zb[(size_t)u * Qr + v];
                bad |= !isfinite(zv.x) || !isfinite(zv.y);
                double cm = hypot(zv.x, zv.y);
                int ci = u * Qr + v;
#pragma unroll
                for (int j = 0; j < RV_LMAX; ++j) {   // sorted insert: larger modulus first, a tie to the lower index
                    if (cm > tm[j] || (cm == tm[j] && ci < ti[j])) {
                        const double sm = tm[j];
                        const int si = ti[j];
                        tm[j] = cm;
                        ti[j] = ci;
                        cm = sm;
                        ci = si;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int r = 16 * i + lr;
                const d2 av = (v < Qr && r < rx) ? a.Ar[(size_t)v * rx + r] : make_double2(0.0, 0.0);
                cmma(Tr[i], Ti[i], av, zv);
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) Ts[(16 * i + lk + 4 * q) * RV_TS + lr] = make_double2(Tr[i][q], Ti[i][q]);
        wsync();
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) {
            const int uu = u0 + k0 + lk;
            d2 bv[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int t = 16 * j + lr;
                bv[j] = (uu < Qt && t < tx) ? cconj(a.At[(size_t)uu * tx + t]) : make_double2(0.0, 0.0);
            }
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const d2 av = Ts[(16 * i + lr) * RV_TS + k0 + lk];
#pragma unroll
                for (int j = 0; j < NT; ++j) cmma(Hr[i][j], Hi[i][j], av, bv[j]);
            }
        }
        wsync();
    }
    // ---------------- the L largest of the wave (:86-88), ascending index
    const double zmax = wave_max(tm[0]);
    const bool zbad = __any(bad) || !(zmax > 0.0);
    for (int l = 0; l < L; ++l) {
        const double wm = wave_max(tm[0]);
        const int wi = wave_min_int(tm[0] == wm ? ti[0] : INT_MAX);
        if (ti[0] == wi && tm[0] == wm) {
#pragma unroll
            for (int j = 0; j + 1 < RV_LMAX; ++j) {
                tm[j] = tm[j + 1];
                ti[j] = ti[j + 1];
            }
            tm[RV_LMAX - 1] = -1.0;
            ti[RV_LMAX - 1] = INT_MAX;
        }
        if (lane == 0) s_pick[l] = zbad ? l : wi;
    }
    // ---------------- H_est and H into LDS; global phase (:187-189), MSE_H (:191)
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 16 * i + lk + 4 * q, t = 16 * j + lr;
                if (r < rx && t < tx) Hs[r + rx * t] = make_double2(Hr[i][j][q], Hi[i][j][q]);
            }
    const d2* Gb = a.vecH + b * (size_t)nh;
    bool gbad = false;
    for (int k = lane; k < nh; k += 64) {
        const d2 g = Gb[k];
        gbad |= !isfinite(g.x) || !isfinite(g.y);
        Gs[k] = g;
    }
    wsync();
    double sgg = 0.0, shh = 0.0;
    d2 shg = make_double2(0.0, 0.0);
    for (int k = lane; k < nh; k += 64) {
        const d2 h = Hs[k], g = Gs[k];
        sgg += cabs2(g);
        shh += cabs2(h);
        shg = cadd(shg, cmulc(h, g));
    }
    sgg = wave_sum(sgg);
    shh = wave_sum(shh);
    shg = rv_wave_csum(shg);
    const double ac = hypot(shg.x, shg.y);
    const bool degen = zbad || __any(gbad) || !(sgg > 0.0) || !(shh > 0.0) || !isfinite(shh) || !isfinite(sgg) || !isfinite(ac);
    const d2 pf = (ac > 0.0 && isfinite(ac)) ? make_double2(shg.x / ac, shg.y / ac) : make_double2(1.0, 0.0);
    double mse = 0.0;
    for (int k = lane; k < nh; k += 64) {
        const d2 h = degen ? make_double2(0.0, 0.0) : cmul(Hs[k], pf);
        Hs[k] = h;
        mse += cabs2(csub(h, Gs[k]));
        if (a.Hest) a.Hest[b * (size_t)nh + k] = h;
    }
    const double mse_h = wave_sum(mse) / sgg;

    // ---------------- angles (:101-161): lane 0 orders the short lists
    uint32_t st = 0;
    bool sweep = a.picks != nullptr;
    int pF1 = 0, pW1 = 0, pF2 = 0, pW2 = 0;
    if (sweep) {
        const int32_t* pk = a.picks + 4 * b;
        pF1 = pk[0];
        pW1 = pk[1];
        pF2 = pk[2];
        pW2 = pk[3];
        sweep = pF1 >= 0 && pF1 < a.Mt && pF2 >= 0 && pF2 < a.Mt && pW1 >= 0 && pW1 < a.Mr && pW2 >= 0 && pW2 < a.Mr;
    }
    if (!sweep) st |= ACE_ST_RECEVAL_NOSWEEP;
    wsync();
    if (lane == 0) {
        for (int i = 1; i < L; ++i) {   // ascending index (:88)
            const int p = s_pick[i];
            int j = i - 1;
            for (; j >= 0 && s_pick[j] > p; --j) s_pick[j + 1] = s_pick[j];
            s_pick[j + 1] = p;
        }
        for (int l = 0; l < L; ++l) {
            const int pu = s_pick[l] / Qr, pv = s_pick[l] - pu * Qr;
            s_eD[l] = a.deg_t[pu];
            s_eA[l] = a.deg_r[pv];
            s_tD[l] = a.aod[b * L + l];
            s_tA[l] = a.aoa[b * L + l];   // (:128 is a no-op: not reordered)
        }
        // stable descending insertion sorts (:127, :131); the true quantised angles, which follow the first one
        // (:129-130), feed :135-136 and :139 only, and those feed no output
        for (int i = 1; i < L; ++i) {
            const double d = s_tD[i];
            int j = i - 1;
            for (; j >= 0 && s_tD[j] < d; --j) s_tD[j + 1] = s_tD[j];
            s_tD[j + 1] = d;
        }
        for (int i = 1; i < L; ++i) {
            const double d = s_eD[i], aa = s_eA[i];
            int j = i - 1;
            for (; j >= 0 && s_eD[j] < d; --j) {
                s_eD[j + 1] = s_eD[j];
                s_eA[j + 1] = s_eA[j];
            }
            s_eD[j + 1] = d;
            s_eA[j + 1] = aa;
        }
        double ed = 0.0, ea = 0.0, s1d = 0.0, s1a = 0.0, s2d = 0.0, s2a = 0.0;
        for (int l = 0; l < L; ++l) {
            ed += fabs(s_eD[l] - s_tD[l]);
            ea += fabs(s_eA[l] - s_tA[l]);
            if (sweep) {
                s1d += fabs(a.pk_t[pF1] - s_tD[l]);
                s1a += fabs(a.pk_r[pW1] - s_tA[l]);
                s2d += fabs(a.cen_t[pF2] - s_tD[l]);
                s2a += fabs(a.cen_r[pW2] - s_tA[l]);
            }
        }
        ed /= L, ea /= L, s1d /= L, s1a /= L, s2d /= L, s2a /= L;
        s_sc[0] = tx == 1 ? ea : rx == 1 ? ed : (ed + ea) / 2.0;
        s_sc[1] = tx == 1 ? s1a : rx == 1 ? s1d : (s1d + s1a) / 2.0;
        s_sc[2] = tx == 1 ? s2a : rx == 1 ? s2d : (s2d + s2a) / 2.0;
        double nq = 0.0;
        if (L == 1) {   // (:149-161; one pick, so the sorted and the unsorted lists agree)
            const int pu = s_pick[0] / Qr, pv = s_pick[0] - pu * Qr;
            const double qd = fabs((double)(a.tidx[2 * b] - (a.first_t + pu)));
            const double qa = fabs((double)(a.tidx[2 * b + 1] - (a.first_r + pv)));
            nq = tx == 1 ? qa : rx == 1 ? qd : (qd + qa) / 2.0;
        }
        s_sc[3] = nq;
    }
    wsync();
    // MSE_ARM (:165-183): unit-norm steering vectors, lane = antenna
    double at = 0.0, ar = 0.0;
    for (int l = 0; l < L; ++l) {
        if (lane < tx) at += cabs2(csub(rv_steer(a.kappa, s_tD[l], lane), rv_steer(a.kappa, s_eD[l], lane)));
        if (lane < rx) ar += cabs2(csub(rv_steer(a.kappa, s_tA[l], lane), rv_steer(a.kappa, s_eA[l], lane)));
    }
    at = wave_sum(at) / ((double)tx * L);
    ar = wave_sum(ar) / ((double)rx * L);
    const double mse_arm = tx == 1 ? ar : rx == 1 ? at : (at + ar) / 2.0;

    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    double out[15];
    out[0] = s_sc[3];
    out[1] = s_sc[0];
    out[2] = 1.0;
    out[3] = 1.0;
    for (int c = 4; c < 14; ++c) out[c] = 0.0;
    out[10] = sweep ? s_sc[1] : qnan;
    out[11] = sweep ? s_sc[2] : qnan;
    if (!sweep) out[8] = out[9] = qnan;
    out[14] = 1.0;
    st |= ACE_ST_EVAL_DEGENERATE;
    if (!degen) {
        // ---------------- pass 0: zgesdd(E) -> v1; 1: zgesdd(E^T) -> u1; 2: zgesdd(G) -> vg; 3: zgesdd(G^T) -> ug
        bool ok = true;
        for (int pass = 0; pass < 4; ++pass) {
            const bool tr = pass & 1;
            const d2* src = pass < 2 ? Hs : Gs;
            for (int k = lane; k < nh; k += 64) {
                const int j = k / m, i = k - j * m;
                if (tr) sh.A[j * ld + i] = src[k];
                else sh.A[i * ld + j] = src[k];
            }
            wsync();
            const int pm = tr ? n : m, pn = tr ? m : n;
            ok &= gesdd_vh<RECT>(sh, pm, pn, ld, lane);
            if (lane < pn) {
                const d2 v = sh.X[lane];   // row 0 of Vh
                if (pass == 0) v1[lane] = cconj(v);
                else if (pass == 1) u1[lane] = v;
                else if (pass == 2) vg[lane] = cconj(v);
                else ug[lane] = v;
            }
            wsync();
        }
        for (int k = lane; k < nh; k += 64) {
            const int j = k / m, i = k - j * m;
            sh.A[i * ld + j] = Gs[k];
        }
        wsync();
        // |w_q^H G f_q| with the phase codes in s_qa [m], s_qb [n]
        auto qgain = [&]() {
            d2 tq = make_double2(0.0, 0.0);
            if (lane < m) {
                for (int j = 0; j < n; ++j) tq = cadd(tq, rotk(sh.A[lane * ld + j], s_qb[j]));
                tq = rotk(tq, -s_qa[lane]);
            }
            const d2 ga = rv_wave_csum(tq);
            return hypot(ga.x, ga.y) / sqrt((double)nh);
        };
        // (:212-217, :289-298) the estimate's pair
        if (lane < m) s_qa[lane] = ps_qcode(u1[lane]);
        if (lane < n) s_qb[lane] = ps_qcode(v1[lane]);
        wsync();
        const double gain_ana = qgain();
        wsync();
        // (:196-203) the true channel's pair
        if (lane < m) s_qa[lane] = ps_qcode(ug[lane]);
        if (lane < n) s_qb[lane] = ps_qcode(vg[lane]);
        wsync();
        const double g_percsi = qgain();
        wsync();
        // (:226-229) the steering vectors at the last estimated pair after the sort of :131
        if (lane < m) s_qa[lane] = ps_qcode(rv_steer(a.kappa, s_eA[L - 1], lane));
        if (lane < n) s_qb[lane] = ps_qcode(rv_steer(a.kappa, s_eD[L - 1], lane));
        wsync();
        const double g_aoda = qgain();
        wsync();
        double g_sw1 = 0.0, g_sw2 = 0.0;
        if (sweep) {   // (:232-238) the picked beams of the two patterns: the quantised steering vectors at the centres
            if (lane < m) s_qa[lane] = ps_qcode(rv_steer(a.kappa, a.cen_r[pW1], lane));
            if (lane < n) s_qb[lane] = ps_qcode(rv_steer(a.kappa, a.cen_t[pF1], lane));
            wsync();
            g_sw1 = qgain();
            wsync();
            if (lane < m) s_qa[lane] = ps_qcode(rv_steer(a.kappa, a.cen_r[pW2], lane));
            if (lane < n) s_qb[lane] = ps_qcode(rv_steer(a.kappa, a.cen_t[pF2], lane));
            wsync();
            g_sw2 = qgain();
            wsync();
        }
        // gain_dig and proj_error (:299, :309-317), as evaluate_kernel sums them
        d2 tg = make_double2(0.0, 0.0), t1 = tg;   // rows of G vg, G v1
        const d2 ui = lane < m ? u1[lane] : make_double2(0.0, 0.0);
        if (lane < m)
            for (int j = 0; j < n; ++j) {
                const d2 g = sh.A[lane * ld + j];
                tg = cadd(tg, cmul(g, vg[j]));
                t1 = cadd(t1, cmul(g, v1[j]));
            }
        const d2 vj = lane < n ? v1[lane] : make_double2(0.0, 0.0);
        const d2 vgj = lane < n ? vg[lane] : make_double2(0.0, 0.0);
        const double nu2 = wave_sum(cabs2(ui)), nv2 = wave_sum(cabs2(vj)), nvg2 = wave_sum(cabs2(vgj));
        const double ng2 = wave_sum(cabs2(tg));
        const d2 gd = rv_wave_csum(cmulc(ui, t1));    // u1^H G v1
        const d2 aa = rv_wave_csum(cmulc(ui, tg));    // u1^H t
        const d2 bq = rv_wave_csum(cmulc(vgj, vj));   // vg^H v1
        const double den = nu2 * nv2;
        const d2 ab = cmul(aa, bq);
        const d2 c = make_double2(ab.x / den, ab.y / den);
        double r2 = 0.0;
        if (lane < m) {
            const d2 cu = cmul(c, ui);
            for (int j = 0; j < n; ++j) r2 += cabs2(csub(cmul(tg, cconj(vg[j])), cmul(cu, cconj(v1[j]))));
        }
        r2 = wave_sum(r2);
        const double gain_dig = hypot(gd.x, gd.y) / sqrt(den);
        const double proj_err = sqrt(r2 / (ng2 * nvg2));
        const double s1 = sqrt(ng2 / nvg2);   // ||G vg|| / ||vg||: the largest singular value of H
        const double np = a.noise_power;
        double o2[15];
        o2[2] = mse_arm;
        o2[3] = mse_h;
        o2[4] = rv_rate(s1, L, np);
        o2[5] = rv_rate(g_percsi, L, np);
        o2[6] = rv_rate(gain_ana, L, np);
        o2[7] = rv_rate(g_aoda, L, np);
        o2[8] = sweep ? rv_rate(g_sw1, L, np) : 0.0;
        o2[9] = sweep ? rv_rate(g_sw2, L, np) : 0.0;
        o2[12] = gain_ana;
        o2[13] = gain_dig;
        o2[14] = proj_err;
        bool fin = true;
        for (int c2 = 2; c2 < 15; ++c2)
            if (c2 != 10 && c2 != 11) fin &= isfinite(o2[c2]);
        if (fin) {
            for (int c2 = 2; c2 < 15; ++c2)
                if (c2 != 10 && c2 != 11 && (sweep || (c2 != 8 && c2 != 9))) out[c2] = o2[c2];
            st = (st & ~ACE_ST_EVAL_DEGENERATE) | (ok ? 0u : ACE_ST_BF_NOCONV);
        }
    }
    if (lane == 0) {
        for (int c = 0; c < 15; ++c) a.metrics[15 * b + c] = out[c];
        if (a.status) a.status[b] = st;
    }
}

// MyBeamSweeping.m:134-154: the first angle of -90 : 0.005 : 90 that maximises |f^H a(theta)|, a the unnormalised
// steering vector.  One block per beam; a thread keeps the first maximum of its stride, the block the first of those.
__global__ __launch_bounds__(PK_NT) void peak_kernel(int N, double kappa, const d2* __restrict__ beams,
                                                     double* __restrict__ out) {
    __shared__ d2 fs[BF_NMAX];
    __shared__ double bg[PK_NT];
    __shared__ int bi[PK_NT];
    const int tid = threadIdx.x;
    const size_t mb = blockIdx.x;
    if (tid < N) fs[tid] = beams[mb * N + tid];
    __syncthreads();
    double best = -1.0;
    int besti = INT_MAX;
    for (int i = tid; i < PK_NANG; i += PK_NT) {
        // MATLAB's colon builds the vector from both ends
        const double ang = i <= PK_NANG / 2 ? -90.0 + 0.005 * i : 90.0 - 0.005 * (PK_NANG - 1 - i);
        const double ks = kappa * sin(ang * kDeg);
        d2 acc = make_double2(0.0, 0.0);
        for (int k = 0; k < N; ++k) {
            const double ph = ks * (double)k;
            acc = cadd(acc, cmulc(fs[k], make_double2(cos(ph), -sin(ph))));
        }
        const double g = hypot(acc.x, acc.y);
        if (g > best) {
            best = g;
            besti = i;
        }
    }
    bg[tid] = best;
    bi[tid] = besti;
    __syncthreads();
    for (int s = PK_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double g2 = bg[tid + s];
            const int i2 = bi[tid + s];
            if (g2 > bg[tid] || (g2 == bg[tid] && i2 < bi[tid])) {
                bg[tid] = g2;
                bi[tid] = i2;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int i = bi[0];
        // (a beam with a non-finite entry never compares greater: NaN marks it)
        out[mb] = i == INT_MAX ? __longlong_as_double(0x7ff8000000000000LL)
                               : (i <= PK_NANG / 2 ? -90.0 + 0.005 * i : 90.0 - 0.005 * (PK_NANG - 1 - i));
    }
}

size_t rv_lds_bytes(int N, bool rect) {
    const size_t nt = (N + 15) / 16;
    return (size_t)(rect ? 3 : 2) * N * (N + 1) * sizeof(d2) + 5 * BF_NMAX * sizeof(d2) + 2 * BF_NMAX * sizeof(double) +
           2 * (size_t)N * N * sizeof(d2) + nt * 16 * RV_TS * sizeof(d2);
}

int rv_check_args(int batch, int tx, int rx, int L, int Qt, int Qr, const void* A_t, const void* A_r, const void* deg_t,
                  const void* deg_r, int first_t, int first_r, double noise_power, double kappa, const void* z,
                  const void* vecH, const void* aod, const void* aoa, const void* tidx, const void* picks, int Mt, int Mr,
                  const void* cen_t, const void* cen_r, const void* pk_t, const void* pk_r, const void* metrics) {
    if (batch < 1) return fail(ACE_ERR_ARG, "evaluate_recovery: batch %d < 1", batch);
    if (tx < 1 || rx < 1) return fail(ACE_ERR_ARG, "evaluate_recovery: %d x %d antennas below 1", tx, rx);
    if (tx > BF_NMAX) return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: tx %d above %d", tx, BF_NMAX);
    if (rx > BF_NMAX) return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: rx %d above %d", rx, BF_NMAX);
    if (L < 1) return fail(ACE_ERR_ARG, "evaluate_recovery: L %d < 1", L);
    if (L > RV_LMAX) return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: L %d above %d", L, RV_LMAX);
    if (Qt < 1 || Qr < 1) return fail(ACE_ERR_ARG, "evaluate_recovery: grid %d x %d below 1", Qt, Qr);
    if (Qt > RV_QMAX) return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: Qt %d above %d", Qt, RV_QMAX);
    if (Qr > RV_QMAX) return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: Qr %d above %d", Qr, RV_QMAX);
    if ((long long)Qt * Qr < L) return fail(ACE_ERR_ARG, "evaluate_recovery: L %d above the grid's %d x %d atoms", L, Qt, Qr);
    if (first_t < 0 || first_r < 0) return fail(ACE_ERR_ARG, "evaluate_recovery: negative first index (%d, %d)", first_t, first_r);
    if (!(noise_power > 0.0) || !std::isfinite(noise_power))
        return fail(ACE_ERR_ARG, "evaluate_recovery: noise_power must be positive and finite");
    if (!(kappa > 0.0) || !std::isfinite(kappa)) return fail(ACE_ERR_ARG, "evaluate_recovery: kappa must be positive and finite");
    const struct {
        const void* p;
        const char* name;
    } req[] = {{A_t, "A_t"}, {A_r, "A_r"}, {deg_t, "deg_t"}, {deg_r, "deg_r"}, {z, "z"}, {vecH, "vecH"},
               {aod, "aod_deg"}, {aoa, "aoa_deg"}, {tidx, "true_idx"}, {metrics, "metrics"}};
    for (const auto& r : req)
        if (!r.p) return fail(ACE_ERR_ARG, "evaluate_recovery: NULL %s", r.name);
    if (picks) {
        if (Mt < 1 || Mr < 1) return fail(ACE_ERR_ARG, "evaluate_recovery: sweep picks with Mt %d, Mr %d below 1", Mt, Mr);
        if (Mt > RV_MMAX || Mr > RV_MMAX)
            return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: Mt %d, Mr %d above %d", Mt, Mr, RV_MMAX);
        if (!cen_t || !cen_r || !pk_t || !pk_r)
            return fail(ACE_ERR_ARG, "evaluate_recovery: sweep picks need the centre_deg and peak_deg tables");
    }
    return ACE_OK;
}

int pk_check_args(int M, int N, double kappa, const void* beams, const void* out) {
    if (M < 1) return fail(ACE_ERR_ARG, "beam_peak_angles: M %d < 1", M);
    if (N < 1) return fail(ACE_ERR_ARG, "beam_peak_angles: N %d < 1", N);
    if (N > BF_NMAX) return fail(ACE_ERR_UNSUPPORTED, "beam_peak_angles: N %d above %d", N, BF_NMAX);
    if (!(kappa > 0.0) || !std::isfinite(kappa)) return fail(ACE_ERR_ARG, "beam_peak_angles: kappa must be positive and finite");
    if (!beams || !out) return fail(ACE_ERR_ARG, "beam_peak_angles: NULL %s", !beams ? "beams" : "peak_deg");
    return ACE_OK;
}

template <bool RECT, int NT>
int rv_launch(int batch, size_t lds, hipStream_t st, const RvArgs& a) {
    const void* kern = (const void*)receval_kernel<RECT, NT>;
    if (!lds_ok(kern, lds))
        return fail(ACE_ERR_UNSUPPORTED, "evaluate_recovery: receval_kernel needs %zu B of dynamic LDS, budget %zu B", lds,
                    lds_dyn_budget(kern));
    hipLaunchKernelGGL((receval_kernel<RECT, NT>), dim3(batch), dim3(64), lds, st, a);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

}  // namespace

size_t receval_request_bytes(int N, int rect) {
    N = N < 1 ? 1 : N > BF_NMAX ? BF_NMAX : N;
    return rv_lds_bytes(N, rect != 0);
}

}  // namespace ace

using namespace ace;

extern "C" int ace_evaluate_recovery_batch(int batch, int tx, int rx, int L, int Qt, int Qr, const double* A_t,
                                           const double* A_r, const double* deg_t, const double* deg_r, int first_t,
                                           int first_r, double noise_power, double kappa, const double* z,
                                           const double* vecH, const double* aod_deg, const double* aoa_deg,
                                           const int32_t* true_idx, const int32_t* picks, int Mt, int Mr,
                                           const double* centre_deg_t, const double* centre_deg_r,
                                           const double* peak_deg_t, const double* peak_deg_r, double* metrics,
                                           double* H_est, uint32_t* status, void* stream) {
    g_err.clear();
    ACE_TRY(rv_check_args(batch, tx, rx, L, Qt, Qr, A_t, A_r, deg_t, deg_r, first_t, first_r, noise_power, kappa, z, vecH,
                          aod_deg, aoa_deg, true_idx, picks, Mt, Mr, centre_deg_t, centre_deg_r, peak_deg_t, peak_deg_r,
                          metrics));
    RvArgs a;
    a.tx = tx, a.rx = rx, a.L = L, a.Qt = Qt, a.Qr = Qr, a.first_t = first_t, a.first_r = first_r;
    a.Mt = picks ? Mt : 0, a.Mr = picks ? Mr : 0;
    a.noise_power = noise_power, a.kappa = kappa;
    a.At = (const d2*)A_t, a.Ar = (const d2*)A_r, a.deg_t = deg_t, a.deg_r = deg_r;
    a.z = (const d2*)z, a.vecH = (const d2*)vecH, a.aod = aod_deg, a.aoa = aoa_deg, a.tidx = true_idx, a.picks = picks;
    a.cen_t = centre_deg_t, a.cen_r = centre_deg_r, a.pk_t = peak_deg_t, a.pk_r = peak_deg_r;
    a.metrics = metrics, a.Hest = (d2*)H_est, a.status = status;
    const int N = std::max(tx, rx);
    const bool rect = tx != rx;
    const size_t lds = rv_lds_bytes(N, rect);
    const hipStream_t st = (hipStream_t)stream;
    if (N <= 16) return rect ? rv_launch<true, 1>(batch, lds, st, a) : rv_launch<false, 1>(batch, lds, st, a);
    return rect ? rv_launch<true, 2>(batch, lds, st, a) : rv_launch<false, 2>(batch, lds, st, a);
}

extern "C" int ace_evaluate_recovery_host(int batch, int tx, int rx, int L, int Qt, int Qr, const double* A_t,
                                          const double* A_r, const double* deg_t, const double* deg_r, int first_t,
                                          int first_r, double noise_power, double kappa, const double* z,
                                          const double* vecH, const double* aod_deg, const double* aoa_deg,
                                          const int32_t* true_idx, const int32_t* picks, int Mt, int Mr,
                                          const double* centre_deg_t, const double* centre_deg_r,
                                          const double* peak_deg_t, const double* peak_deg_r, double* metrics,
                                          double* H_est, uint32_t* status) {
    g_err.clear();
    ACE_TRY(rv_check_args(batch, tx, rx, L, Qt, Qr, A_t, A_r, deg_t, deg_r, first_t, first_r, noise_power, kappa, z, vecH,
                          aod_deg, aoa_deg, true_idx, picks, Mt, Mr, centre_deg_t, centre_deg_r, peak_deg_t, peak_deg_r,
                          metrics));
    const size_t B = batch, nh = (size_t)tx * rx, nz = (size_t)Qt * Qr;
    DevScope d;
    double *dAt, *dAr, *ddt, *ddr, *dz, *dH, *daod, *daoa, *dmet, *dHe = nullptr;
    double *dct = nullptr, *dcr = nullptr, *dpt = nullptr, *dpr = nullptr;
    int32_t *dti, *dpk = nullptr;
    uint32_t* dst;
    ACE_TRY(d.put(&dAt, A_t, 2 * (size_t)Qt * tx));
    ACE_TRY(d.put(&dAr, A_r, 2 * (size_t)Qr * rx));
    ACE_TRY(d.put(&ddt, deg_t, (size_t)Qt));
    ACE_TRY(d.put(&ddr, deg_r, (size_t)Qr));
    ACE_TRY(d.put(&dz, z, 2 * B * nz));
    ACE_TRY(d.put(&dH, vecH, 2 * B * nh));
    ACE_TRY(d.put(&daod, aod_deg, B * L));
    ACE_TRY(d.put(&daoa, aoa_deg, B * L));
    ACE_TRY(d.put(&dti, true_idx, 2 * B * L));
    if (picks) {
        ACE_TRY(d.put(&dpk, picks, 4 * B));
        ACE_TRY(d.put(&dct, centre_deg_t, (size_t)Mt));
        ACE_TRY(d.put(&dcr, centre_deg_r, (size_t)Mr));
        ACE_TRY(d.put(&dpt, peak_deg_t, (size_t)Mt));
        ACE_TRY(d.put(&dpr, peak_deg_r, (size_t)Mr));
    }
    ACE_TRY(d.alloc(&dmet, 15 * B));
    ACE_TRY(d.alloc(&dst, B));
    if (H_est) ACE_TRY(d.alloc(&dHe, 2 * B * nh));
    ACE_TRY(ace_evaluate_recovery_batch(batch, tx, rx, L, Qt, Qr, dAt, dAr, ddt, ddr, first_t, first_r, noise_power, kappa,
                                        dz, dH, daod, daoa, dti, dpk, Mt, Mr, dct, dcr, dpt, dpr, dmet, dHe, dst, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(d.get(metrics, dmet, 15 * B));
    ACE_TRY(d.get(H_est, dHe, 2 * B * nh));
    return d.get(status, dst, B);
}

extern "C" int ace_beam_peak_angles(int M, int N, double kappa, const double* beams, double* peak_deg, void* stream) {
    g_err.clear();
    ACE_TRY(pk_check_args(M, N, kappa, beams, peak_deg));
    hipLaunchKernelGGL(peak_kernel, dim3(M), dim3(PK_NT), 0, (hipStream_t)stream, N, kappa, (const d2*)beams, peak_deg);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_beam_peak_angles_host(int M, int N, double kappa, const double* beams, double* peak_deg) {
    g_err.clear();
    ACE_TRY(pk_check_args(M, N, kappa, beams, peak_deg));
    DevScope d;
    double *db, *dout;
    ACE_TRY(d.put(&db, beams, 2 * (size_t)M * N));
    ACE_TRY(d.alloc(&dout, (size_t)M));
    ACE_TRY(ace_beam_peak_angles(M, N, kappa, db, dout, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    return d.get(peak_deg, dout, (size_t)M);
}
