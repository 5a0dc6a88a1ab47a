// Batched PR-GAMP against one shared matrix D [m][N]: the PRGAMP baseline of Vs_M.m (MyCPR.m:110-120 ->
// MyPRGAMP.m:71 -> prGAMP4(sqrt(y), A, opt_pr)), compressive phase retrieval straight from the magnitudes.  The
// reference vendors the solver (3rd_software_component/GAMP/trunk/code: phase/prGAMP4.m, phase/ncCAwgnEstimOut.m,
// main/gampEst.m, main/estimInvert.m, main/CAwgnEstimIn.m, main/SparseScaEstim.m, main/GampOpt.m); this restates what
// those files do for the option set of MyCPR.m, T = 1 column per realisation.  The sibling is csrc/ace_gamp.hip
// (EM-BG-GAMP): the layout, the sweeps, the reductions and the idle-when-stopped columns are its.
//
// Options (prGAMP4.m:250-459 from MyCPR.m:110-120): xreal 0, xnonneg 0, tuneOn 1 (sparseRat <- min(sparseRat, 0.9),
// :438), EMtype 0, init_gain 100, maxTol 1e-4, minTry 1, sparseRatTry inf; gampEst: adaptStep, adaptStepBethe,
// step = stepMax = 0.25, stepMin 0.05, stepWindow 50, stepIncr 1.1, stepDecr 0.2, varNorm, pvarStep, no rvarStep, no
// uniformVariance.  Of GampOpt's defaults these matter: stepTol 1e-10 (never reached: stepMin is above it),
// maxBadSteps inf (the fail count is not kept), pvarMin = xvarMin 1e-12 (pvarRobust, rvarRobust), zvarToPvarMax inf
// (a min that only turns a NaN zvar / pvar into inf, as MATLAB's min skips NaN).  In the cfg: sparse_rat, snr_db_init,
// snr_db, max_try, nit_em, gamp_nit.
//
// One kernel, one launch: every try (prGAMP4.m:598-903), every EM iteration (:639-747) and every GAMP iteration
// (gampEst.m:403-653).  A work-group (8 waves) owns PG_RB = 16 realisations, the columns of one MFMA tile, and runs
// them to the end.  A realisation that has left a loop (estimInvert's, a gampEst call, everything) idles with its
// state frozen; the group leaves the loop when all 16 have.  Control state is per realisation: thread t serves
// realisation t & 15 in every phase and the 32 threads of a realisation hold identical copies, computed from the
// same reduced sums.  Nothing is combined across work-groups; there are no atomics; every sum has a fixed order
// (per thread in index order, then the 32 partials in thread order, the waves' tiles in wave order), so a
// realisation's outputs are a function of (y_b, G_b, D, cfg, m, N) alone.
//
// A GAMP iteration (gampEst.m:403-653):
//   forward sweep   Axhat = D xhat (4M complex product) and A2xvar = |D|^2 xvar on v_mfma_f64_16x16x4_f64 (cmma /
//                   mfma64 of ace_mfma.hpp), as in gamp_kernel.
//   m-space         pvar = (1 - step) pvarOpt + step A2xvar (:434-445; A2xvar and pvar are one vector: no matrix
//                   uncertainty), phat = Axhat - ((1 / scaleFac) pvar) shat (:448), pvarRobust = max(pvar, 1e-12);
//                   the Bethe cost ncCAwgnEstimOut.logScale (:132-170): estimInvert (alg 1, maxIter 25, tol 1e-6,
//                   stepsize 0.95, regularization 0, phat0 = Axhat; its stop tests are norms over the realisation's
//                   m-vector, up to ten attempts at a fifth of the step size while NR > 1.01 NR0), from the second
//                   EM iteration on tune (:77-101: the object is a handle, var0 really changes, on failed iterations
//                   too, and before the cost is formed), then the sum of the cost with log I0e of ace_bessel.hpp;
//                   val = that + valIn; the pass test against the minimum of the last stepWindow + 1 passed utilities
//                   (:467-471; fmin: MATLAB's min skips NaN), forced on the first iteration of a call and at
//                   step <= stepMin.  On a pass: the Opt copies, the exports, scaleFac = mean(pvarRobust) (:541-548),
//                   ncCAwgnEstimOut.estim with the Amos bounds (:60-68), shatNew, svarNew, the step increase; else
//                   the decrease.  Damping of shat / svar (|svar| < eps becomes eps) into LDS, the B operand of the
//   backward sweep  D^H shat and |D|^2^T svar, raw sums to the workspace.
//   N-space         (before the sweep) on a pass the Opt copies, xhatFinal, rhatFinal, rvarFinal = rvarOpt scaleFac
//                   (the scaleFac of before this pass, :506) and the sums of the tolerance test (:513); xhatDamp.
//                   (after it) rvar, rhat, rvarRobust scaleFac (:646), SparseScaEstim.estim around CAwgnEstimIn.estim
//                   in two passes over the atoms, as the tuning needs: py1 from the old p1, p1 <- mean(py1),
//                   mixWeight = py1 / p1; then var0 <- mean(mixWeight |xhat1|^2 + xvar1) with xhat1, xvar1 and the KL
//                   term from the old var0 and the KL's prior terms from the new p1.  disableTune holds during the
//                   first EM iteration (prGAMP4.m:654-671); both counter fields are 0 and nothing sets them.
// The first pass of EVERY call exports rhat = rvar = NaN (gampEst.m:362-363 declares them per call), so a call with one
// pass fails the isnonzero test of prGAMP4.m:722.
//
// Warm start between EM iterations (GampOpt.warmStart): xhatNext, xvarNext, xhatDamp, pvarOpt = A2xvarOpt, scaleFac,
// step, valIn and the whole list of passed utilities stay where they are; shat and svar go through
// (v / scaleFac) scaleFac (shatNext of gampEst.m:658, shat0 scaleFac of :254); rhat, rvar and xhatFinal start over.
// tolGAMP = min(10^(-SNRdB_hat / 10), maxTol), tolEM = 10 tolGAMP, wvar_hat(em + 1) = mean(var0) = what the last
// call left.  Misconvergence (:722-728) doubles init_gain and shrinks stepWindow to ceil(0.75 .) for all later tries.
// Per try: the tuned prior restored (:614-623), xhat0 = init_gain sqrt(sparseRat xvar0 / 2) G (:608-611; G is the
// caller's, MATLAB's randn stream cannot be reproduced), xvar0 of gampEst = mean |xhat0|^2 (:613), the best residual
// kept (:867-876), the stop at nresGAMPdB_best < -(SNRdB + 2) with the posterior support count (:879-901;
// sparseRatTry = inf never rejects).  out.sparseRat_hat / xvar0_hat are those of the LAST try (:914-915).
//
// What raises in the reference (MyPRGAMP's catch returns zeros), and so sets ACE_ST_PRGAMP_FAILED with xhat zeroed:
//   - CAwgnEstimIn's assert(all(var0 > 0)) at construction: xvar0 0 (y = 0) or NaN;
//   - the same assert in the tuning of var0 (CAwgnEstimIn.m:130 through set.var0): a tuned var0 that is NaN or <= 0;
//   - prGAMP4.m:909 reads estFin_best, never assigned when every try ends with a NaN or +Inf residual.  A y whose
//     squared norm overflows gives xvar0 = Inf, every residual NaN or Inf, and ends there: xvar0 = Inf is taken
//     straight to the failure.
// (opt_pr.sparseRat outside (0, 1] raises too: that is an argument error here.)
//
// Workspace per work-group, [index][16 realisations]: 23 doubles per atom (184 B per atom and realisation) and 24
// per row rounded up to 16 (192 B).  The restart draws are the caller's: G [batch][max_try][N] complex.
// LDS: dynamic max(8 x 32 x 16 x 3 doubles of forward partials, 16 (MP + 1) x 24 B of shat / svar) = 98304 B up to
// m = 240 and 98688 B at m = 256, through the derived budget (lds_dyn_budget); static 27904 B: the reductions, the
// window of passed utilities (64 x 16 doubles) and the realisations' scalars.  254 VGPRs (two waves per SIMD), no VGPR
// spill and no scratch; the scalar side parks 87 values in the lanes of a VGPR, as gamp_kernel does.  That took, on top
// of what gamp_kernel does (the opaque copies of the lane, wave and thread indices and of the workspace base, renewed
// per phase): the scalars that live across the sweeps (noise variance, p1, var0, valIn, step, scaleFac, the tolerance,
// the window's counters, the try-level bookkeeping) in LDS, written by the realisation's first thread and read after a
// barrier; the persistent flags in one word; N, m and the prior odds as double arguments (the conversions and the
// division were hoisted out of the main loop and kept); opaque indices in the try set-up too.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"
#include "ace_bessel.hpp"

#include <cmath>

namespace ace {
namespace {

constexpr int PG_WAVES = 8;
constexpr int PG_NT = 64 * PG_WAVES;
constexpr int PG_RB = 16;               // realisations per work-group (the columns of one MFMA tile)
constexpr int PG_TR = PG_NT / PG_RB;    // threads of a realisation
constexpr int PG_MMAX = 256;
constexpr int PG_NMAX = 16384;
constexpr int PG_RT = 2;                // row tiles of the forward sweep per pass (32 rows)
constexpr int PG_TW = 2;                // atom tiles per wave and pass of the backward sweep
constexpr int PG_SK = 4;                // k-steps per chunk
constexpr int PG_RK = 4;                // sums per reduction
constexpr int PG_WIN = 64;              // ring of passed utilities (stepWindow + 1 = 51 are read)
constexpr int PG_NV = 23;               // doubles per atom
constexpr int PG_MV = 24;               // doubles per row
constexpr double PG_EPS = 0x1p-52;
static_assert(PG_TR == 32 && PG_RT * 16 == PG_TR, "thread layout");

struct PrGampArgs {
    int batch, m, N, max_try, nit_em, nit;
    double sr;              // min(sparse_rat, 0.9)
    double snr, snri;       // 10^(min(100, SNRdB) / 10), the same of SNRdBinit
    double stopdb;          // -(min(100, SNRdB) + 2)
    double odds;            // (1 - sr) / sr of the posterior support probabilities
    double Nd, md;          // N and m as doubles (kernel arguments: nothing for the compiler to hoist and keep)
    const d2* D;
    const double* Y;
    const d2* G;
    d2* xhat;
    double* info;
    int32_t* counts;
    uint32_t* status;
    int32_t* trace;
    double* vals;
    double* ws;
};

constexpr size_t pg_lds_bytes(int m) {
    const size_t part = (size_t)PG_WAVES * PG_TR * PG_RB * 3 * sizeof(double);
    const size_t opnd = (size_t)PG_RB * ((m + 15) / 16 * 16 + 1) * (sizeof(d2) + sizeof(double));
    return part > opnd ? part : opnd;
}
constexpr size_t pg_group_doubles(int m, int N) {
    return (size_t)PG_NV * N * PG_RB + (size_t)PG_MV * ((m + 15) / 16 * 16) * PG_RB;
}

// |a|^2 in one fixed form (see ga_abs2_rn of ace_gamp.hip)
__device__ __forceinline__ double pg_abs2(d2 a) {
    const double yy = a.y * a.y;
    return __builtin_fma(a.x, a.x, yy);
}

__device__ __forceinline__ double pg_pick(const d4v (&v)[PG_TW], int cq) {
    double r = v[0][0];
#pragma unroll
    for (int c = 0; c < PG_TW; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) r = cq == 4 * c + q ? v[c][q] : r;
    return r;
}

// v[k] <- the sum over the 32 threads of the realisation, in thread order: the same bits in all of them
template <int K>
__device__ __forceinline__ void pg_red(double (&v)[K], double* red, int t) {
    static_assert(K <= PG_RK, "reduction buffer");
#pragma unroll
    for (int k = 0; k < K; ++k) red[(k * PG_TR + (t >> 4)) * PG_RB + (t & 15)] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < PG_TR; ++i) s += red[(k * PG_TR + i) * PG_RB + (t & 15)];
        v[k] = s;
    }
    __syncthreads();
}

// ncCAwgnEstimOut.estim (:48-74): the posterior of z ~ CN(phat, pvar) given |z + w| = y, w ~ CN(0, wv)
__device__ __forceinline__ void pg_estim(double y, d2 p, double pv, double wv, d2& zh, double& zv) {
    const double pa = sqrt(pg_abs2(p));
    const double B = 2.0 * y * pa / (wv + pv);
    const double r = bessel_i1i0_amos(B);
    const double ysca = y / (1.0 + wv / pv);
    const double psca = pa / (1.0 + pv / wv);
    const double mag = psca + ysca * r;
    const d2 sg = pa == 0.0 ? make_double2(0.0, 0.0) : make_double2(p.x / pa, p.y / pa);
    zh = cscale(sg, mag);
    zv = ysca * ysca + psca * psca + (1.0 + B * r) / (1.0 / wv + 1.0 / pv) - pg_abs2(zh);
}

// The vectors of the work-group's workspace, declared where a phase uses them (see GA_VECS of ace_gamp.hip).
#define PG_VECS(wsb_, nN_, nM_) \
    double* gq_ = (wsb_); \
    size_t gn_ = (nN_), gm_ = (nM_); \
    asm volatile("" : "+s"(gq_), "+s"(gn_), "+s"(gm_)); \
    [[maybe_unused]] d2* const XH = (d2*)(gq_ + 0 * gn_); /* xhat */ \
    [[maybe_unused]] d2* const XD = (d2*)(gq_ + 2 * gn_); /* xhatDamp */ \
    [[maybe_unused]] d2* const XO = (d2*)(gq_ + 4 * gn_); /* xhatOpt = xhatFinal */ \
    [[maybe_unused]] d2* const XDO = (d2*)(gq_ + 6 * gn_); /* xhatDampOpt */ \
    [[maybe_unused]] d2* const RH = (d2*)(gq_ + 8 * gn_); /* rhat (the raw D^H shat between sweep and N-space) */ \
    [[maybe_unused]] d2* const RHF = (d2*)(gq_ + 10 * gn_); /* rhatFinal */ \
    [[maybe_unused]] d2* const XP = (d2*)(gq_ + 12 * gn_); /* xhat_old of the EM loop */ \
    [[maybe_unused]] d2* const XB = (d2*)(gq_ + 14 * gn_); /* estFin_best.xhat */ \
    [[maybe_unused]] d2* const RHB = (d2*)(gq_ + 16 * gn_); /* estFin_best.rhat */ \
    [[maybe_unused]] double* const XV = (double*)(gq_ + 18 * gn_); /* xvar */ \
    [[maybe_unused]] double* const RV = (double*)(gq_ + 19 * gn_); /* rvar (raw |D|^2^T svar likewise) */ \
    [[maybe_unused]] double* const RVF = (double*)(gq_ + 20 * gn_); /* rvarFinal */ \
    [[maybe_unused]] double* const RVB = (double*)(gq_ + 21 * gn_); /* estFin_best.rvar */ \
    [[maybe_unused]] double* const PY = (double*)(gq_ + 22 * gn_); /* py1 */ \
    double* const gr_ = gq_ + PG_NV * gn_; \
    [[maybe_unused]] double* const YM = (double*)(gr_ + 0 * gm_); /* abs_y */ \
    [[maybe_unused]] d2* const SH = (d2*)(gr_ + 1 * gm_); /* shat */ \
    [[maybe_unused]] d2* const SHO = (d2*)(gr_ + 3 * gm_); /* shatOpt */ \
    [[maybe_unused]] d2* const SHN = (d2*)(gr_ + 5 * gm_); /* shatNew */ \
    [[maybe_unused]] d2* const AX = (d2*)(gr_ + 7 * gm_); /* Axhat */ \
    [[maybe_unused]] d2* const AXF = (d2*)(gr_ + 9 * gm_); /* AxhatFinal */ \
    [[maybe_unused]] d2* const PH = (d2*)(gr_ + 11 * gm_); /* phat */ \
    [[maybe_unused]] d2* const PF = (d2*)(gr_ + 13 * gm_); /* estimInvert's phat */ \
    [[maybe_unused]] d2* const ZH = (d2*)(gr_ + 15 * gm_); /* estimInvert's zhat */ \
    [[maybe_unused]] double* const SV = (double*)(gr_ + 17 * gm_); /* svar */ \
    [[maybe_unused]] double* const SVO = (double*)(gr_ + 18 * gm_); /* svarOpt */ \
    [[maybe_unused]] double* const SVN = (double*)(gr_ + 19 * gm_); /* svarNew */ \
    [[maybe_unused]] double* const A2 = (double*)(gr_ + 20 * gm_); /* A2xvar as the sweep left it */ \
    [[maybe_unused]] double* const PV = (double*)(gr_ + 21 * gm_); /* pvar (stepped) */ \
    [[maybe_unused]] double* const PVO = (double*)(gr_ + 22 * gm_); /* pvarOpt */ \
    [[maybe_unused]] double* const ZV = (double*)(gr_ + 23 * gm_); /* estimInvert's zvar */

// try-level scalars of a realisation, kept in LDS (written by the realisation's thread 0, read after a barrier)
enum { PS_XVAR0, PS_GAIN, PS_BEST, PS_BWV, PS_BSNR, PS_LP1, PS_LVX, PS_WINIT, PS_MY2, PS_NY2,
       PS_WV, PS_WVS, PS_P1, PS_VX, PS_VALIN, PS_VALP, PS_STEP, PS_SF, PS_TOL2, PS_COUNT };   // from PS_WV on: the call-level state (noise variance,
                                                                     // its value at the call's entry, p1, var0, valIn, the last passed val)
enum { PI_WINDOW, PI_BT, PI_BEM, PI_SUPP, PI_HAVE, PI_WN, PI_WTRY, PI_NPASS, PI_COUNT };

__global__ __launch_bounds__(PG_NT) void prgamp_kernel(const PrGampArgs a) {
    extern __shared__ __align__(16) unsigned char pg_lds[];   // forward partials | shat, svar operands (pg_lds_bytes)
    __shared__ double red[PG_RK * PG_TR * PG_RB];
    __shared__ double sb[PG_RB];
    __shared__ double win[PG_WIN][PG_RB];
    __shared__ double ps[PS_COUNT][PG_RB];
    __shared__ int pi[PI_COUNT][PG_RB];
    const int m = a.m, N = a.N;
    const int MP = (m + 15) / 16 * 16, ST = MP + 1;
    double* const part = (double*)pg_lds;
    d2* const shL = (d2*)pg_lds;
    double* const svL = (double*)(shL + PG_RB * ST);
    const d2* __restrict__ const D = a.D;

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bc = t & 15, tr = t >> 4;
    const long long b = (long long)blockIdx.x * PG_RB + bc;
    const bool live = b < a.batch;

    const size_t nN = (size_t)N * PG_RB, nM = (size_t)MP * PG_RB;
    double* const wsb = a.ws + (size_t)blockIdx.x * pg_group_doubles(m, N);

    // ---------------- A_fro_2 = sum |D|^2 (prGAMP4.m:364), abs_y, ||abs_y||^2
    double dsum;
    {
        double v[1] = {0.0};
        for (size_t i = t; i < (size_t)m * N; i += PG_NT) v[0] += cabs2(D[i]);
        pg_red(v, red, t);
        if (tr == 0) sb[bc] = v[0];
        __syncthreads();
        dsum = 0.0;
        for (int i = 0; i < PG_RB; ++i) dsum += sb[i];
    }
    uint32_t stat = 0u;
    {
        double v[2] = {0.0, 0.0};
        PG_VECS(wsb, nN, nM)
        for (int e = tr; e < MP; e += PG_TR) {
            double y = 0.0;
            if (live && e < m) y = a.Y[(size_t)b * m + e];
            if (!isfinite(y)) v[1] += 1.0;
            y = fabs(y);
            v[0] += y * y;
            YM[e * PG_RB + bc] = y;
        }
        pg_red(v, red, t);
        const double ny2 = v[0];
        const double my2 = ny2 / a.md;
        const double xvar0 = ny2 * a.snr / (a.snr + 1.0) / a.sr / dsum;
        if (v[1] != 0.0) stat = ACE_ST_EVAL_DEGENERATE;
        else if (!(xvar0 > 0.0 && xvar0 < INFINITY)) stat = ACE_ST_PRGAMP_FAILED;
        if (tr == 0) {
            ps[PS_XVAR0][bc] = xvar0;
            ps[PS_GAIN][bc] = 100.0;
            ps[PS_BEST][bc] = INFINITY;
            ps[PS_BWV][bc] = 0.0;
            ps[PS_BSNR][bc] = 0.0;
            ps[PS_LP1][bc] = 0.0;
            ps[PS_LVX][bc] = 0.0;
            ps[PS_WINIT][bc] = my2 / (a.snri + 1.0);
            ps[PS_MY2][bc] = my2;
            ps[PS_NY2][bc] = ny2;
            pi[PI_WINDOW][bc] = 50;
            pi[PI_BT][bc] = 0;
            pi[PI_BEM][bc] = 0;
            pi[PI_SUPP][bc] = -1;
            pi[PI_HAVE][bc] = 0;
        }
        __syncthreads();
    }

    // the realisation's persistent flags in one word (one register across the sweeps)
    enum { F_DONE = 1, F_NEWTRY = 2, F_COLD = 4, F_STOPPED = 8, F_RAISED = 16 };
    int fl = F_NEWTRY | F_COLD | ((!live || stat != 0u) ? F_DONE : 0);
    int ntry = 0, em = 0;
    const int nch = (N + 15) / 16, nrg = (m + PG_TR - 1) / PG_TR;
    const int ntile = nch, npair = (ntile + PG_TW - 1) / PG_TW, nst = MP / (4 * PG_SK);

    while (true) {
        if (__syncthreads_or(!(fl & F_DONE)) == 0) break;
        // ================================================= set up one gampEst call for the realisations not done
        const bool incall = !(fl & F_DONE);
        {
            // a new try (prGAMP4.m:600-636): xhat0 = init_gain sqrt(sparseRat xvar0 / 2) G, xvar0 = mean |xhat0|^2
            int ql = t;   // (opaque copies of the thread's indices, as in the phases below: no address is hoisted out of the loop)
            asm volatile("" : "+v"(ql));
            const int qb = ql & 15, qt = ql >> 4;
            const bool nt = incall && (fl & F_NEWTRY);
            double v[1] = {0.0};
            PG_VECS(wsb, nN, nM)
            if (nt) {
                const double sc = ps[PS_GAIN][qb] * sqrt(a.sr * ps[PS_XVAR0][qb] / 2.0);
                const d2* const g = a.G + ((size_t)((long long)blockIdx.x * PG_RB + qb) * a.max_try + ntry) * N;
                for (int j = qt; j < N; j += PG_TR) {
                    const d2 x0 = cscale(g[j], sc);
                    XH[(size_t)j * PG_RB + qb] = x0;
                    v[0] += pg_abs2(x0);
                }
            }
            pg_red(v, red, t);
            if (nt) {
                const double xv0 = v[0] / a.Nd;
                for (int j = qt; j < N; j += PG_TR) XV[(size_t)j * PG_RB + qb] = xv0;
                for (int e = qt; e < MP; e += PG_TR) SH[e * PG_RB + qb] = make_double2(0.0, 0.0);
                ++ntry;
                em = 0;
                if (qt == 0) {
                    win[0][qb] = -INFINITY;
                    pi[PI_WN][qb] = 1;
                    pi[PI_WTRY][qb] = pi[PI_WINDOW][qb];
                    ps[PS_SF][qb] = 1.0;
                    ps[PS_STEP][qb] = 0.25;
                    ps[PS_P1][qb] = a.sr;
                    ps[PS_VX][qb] = ps[PS_XVAR0][qb];
                    ps[PS_WV][qb] = ps[PS_WINIT][qb];
                    ps[PS_VALIN][qb] = -INFINITY;
                }
                fl = (fl | F_COLD) & ~F_NEWTRY;
            }
        }
        __syncthreads();   // (the new try's stores, the window's first entry)
        {
            // SNRdB_hat(em), tolGAMP (prGAMP4.m:646-647) from the noise variance the last call left
            const double wvs = ps[PS_WV][bc];
            const double snrhat = 10.0 * log10(ps[PS_MY2][bc] / wvs);
            const double tolg = fmin(pow(10.0, -snrhat / 10.0), 1e-4);
            if (tr == 0 && incall) {
                ps[PS_WVS][bc] = wvs;
                ps[PS_VALP][bc] = NAN;
                ps[PS_TOL2][bc] = tolg * tolg;
                pi[PI_NPASS][bc] = 0;
            }
        }
        const bool tune = em >= 1;
        int it = 0;
        bool gstop = !incall;

        while (true) {
            if (__syncthreads_or(!gstop) == 0) break;
            const bool act = !gstop;
            bool stopnow = false;
            if (act) {
                ++it;
                stopnow = it >= a.nit;
            }
            const bool first_cold = it == 1 && (fl & F_COLD);

            int ln = lane;
            asm volatile("" : "+v"(ln));
            int lb = ln & 15, lt = 4 * w + (ln >> 4);   // = bc, tr
            int wf = w;
            asm volatile("" : "+s"(wf));
            // ---------------- forward sweep: Axhat = D xhat, A2xvar = |D|^2 xvar
            for (int rg = 0; rg < nrg; ++rg) {
                PG_VECS(wsb, nN, nM)
                struct FSet {
                    d2 dd[PG_RT][PG_SK];
                };
                d4v cr[PG_RT], ci4[PG_RT], re[PG_RT];
#pragma unroll
                for (int c = 0; c < PG_RT; ++c) cr[c] = ci4[c] = re[c] = d4v{0.0, 0.0, 0.0, 0.0};
                auto fload = [&](FSet& f, int ch) {
#pragma unroll
                    for (int kk = 0; kk < PG_SK; ++kk) {
                        const int j = 16 * ch + 4 * kk + (ln >> 4);
                        const bool in = j < N;
#pragma unroll
                        for (int c = 0; c < PG_RT; ++c) {
                            const int e = PG_TR * rg + 16 * c + (ln & 15);
                            f.dd[c][kk] = make_double2(0.0, 0.0);
                            if (in && e < m) f.dd[c][kk] = D[(size_t)e * N + j];
                        }
                    }
                };
                auto fcomp = [&](const FSet& f, int ch) {
#pragma unroll
                    for (int kk = 0; kk < PG_SK; ++kk) {
                        const int j = 16 * ch + 4 * kk + (ln >> 4);
                        d2 xh = make_double2(0.0, 0.0);
                        double xv = 0.0;
                        if (j < N) {
                            xh = XH[(size_t)j * PG_RB + (ln & 15)];
                            xv = XV[(size_t)j * PG_RB + (ln & 15)];
                        }
#pragma unroll
                        for (int c = 0; c < PG_RT; ++c) {
                            const d2 v = f.dd[c][kk];
                            cmma(cr[c], ci4[c], v, xh);
                            re[c] = mfma64(v.x * v.x + v.y * v.y, xv, re[c]);
                        }
                    }
                };
                FSet fa, fb;
                fload(fa, wf);
                for (int ch = wf; ch < nch; ch += 2 * PG_WAVES) {
                    fload(fb, ch + PG_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                    fcomp(fa, ch);
                    __builtin_amdgcn_sched_barrier(0);
                    fload(fa, ch + 2 * PG_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                    if (ch + PG_WAVES < nch) fcomp(fb, ch + PG_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int c = 0; c < PG_RT; ++c)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        double* const o = part + ((size_t)(wf * PG_TR + 16 * c + (ln >> 4) + 4 * q) * PG_RB + (ln & 15)) * 3;
                        o[0] = cr[c][q];
                        o[1] = ci4[c][q];
                        o[2] = re[c][q];
                    }
                __syncthreads();
                {
                    double sx = 0.0, sy = 0.0, sr = 0.0;
#pragma unroll
                    for (int v = 0; v < PG_WAVES; ++v) {
                        const double* const o = part + ((size_t)(v * PG_TR + lt) * PG_RB + lb) * 3;
                        sx += o[0];
                        sy += o[1];
                        sr += o[2];
                    }
                    const int e = PG_TR * rg + lt;
                    if (act && e < m) {
                        AX[e * PG_RB + lb] = make_double2(sx, sy);
                        A2[e * PG_RB + lb] = sr;
                    }
                }
                __syncthreads();
            }

            // ---------------- m-space: pvar, phat, the first estimate of estimInvert
            asm volatile("" : "+v"(ln));
            lb = ln & 15, lt = 4 * w + (ln >> 4);
            double sfsum, NR0, nz0;
            double wv = ps[PS_WV][lb], step = ps[PS_STEP][lb], sf = ps[PS_SF][lb];
            const int wn = pi[PI_WN][lb], wtry = pi[PI_WTRY][lb];
            {
                PG_VECS(wsb, nN, nM)
                double v[3] = {0.0, 0.0, 0.0};
                if (act)
                    for (int e = lt; e < m; e += PG_TR) {
                        const int i = e * PG_RB + lb;
                        const double a2 = A2[i];
                        const double pvo = first_cold ? a2 : PVO[i];
                        const double pv = (1.0 - step) * pvo + step * a2;
                        const d2 ax = AX[i];
                        PV[i] = pv;
                        PH[i] = csub(ax, cscale(SH[i], (1.0 / sf) * pv));
                        v[0] += fmax(pv, 1e-12);
                        d2 zh;
                        double zv;
                        pg_estim(YM[i], ax, pv, wv, zh, zv);
                        PF[i] = ax;
                        ZH[i] = zh;
                        ZV[i] = zv;
                        v[1] += pg_abs2(csub(ax, zh));
                        v[2] += pg_abs2(zh);
                    }
                pg_red(v, red, t);
                sfsum = v[0];
                NR0 = sqrt(v[1]);
                nz0 = sqrt(v[2]);
            }
            // ---------------- estimInvert (estimInvert.m:48-139)
            {
                double gam = 0.95, NR = NR0, NRold = INFINITY, nz = nz0;
                int r = 0, att = 0;
                bool idone = !act, restart = false;
                while (true) {
                    bool cont = false;
                    if (!idone && !restart) {
                        cont = r < 25 && NR > 1e-6 * nz && fabs(NR - NRold) > 1e-6 * NR;
                        if (!cont) {
                            if (NR > 1.01 * NR0 && att < 9) {
                                gam /= 5.0;
                                ++att;
                                restart = true;
                            } else {
                                idone = true;
                            }
                        }
                    }
                    if (__syncthreads_or(!idone) == 0) break;
                    PG_VECS(wsb, nN, nM)
                    double v[2] = {0.0, 0.0};
                    if (restart || cont)
                        for (int e = lt; e < m; e += PG_TR) {
                            const int i = e * PG_RB + lb;
                            const d2 ax = AX[i];
                            const double pv = PV[i];
                            d2 pf = ax;
                            if (cont) {
                                const d2 res = csub(ax, ZH[i]);
                                const double grad = ZV[i] / pv;
                                const double den = grad * grad + 0.0;
                                const d2 pold = PF[i];
                                pf = make_double2(pold.x + gam * res.x * grad / den, pold.y + gam * res.y * grad / den);
                            }
                            d2 zh;
                            double zv;
                            pg_estim(YM[i], pf, pv, wv, zh, zv);
                            PF[i] = pf;
                            ZH[i] = zh;
                            ZV[i] = zv;
                            v[0] += pg_abs2(csub(ax, zh));
                            v[1] += pg_abs2(zh);
                        }
                    pg_red(v, red, t);
                    if (cont) {
                        ++r;
                        NRold = NR;
                        NR = sqrt(v[0]);
                        nz = sqrt(v[1]);
                    } else if (restart) {
                        r = 0;
                        NR = NR0;
                        NRold = INFINITY;
                        nz = nz0;
                        restart = false;
                    }
                }
            }
            // ---------------- tune (ncCAwgnEstimOut.m:77-101) and the cost (:163-169)
            double val;
            {
                PG_VECS(wsb, nN, nM)
                double v[2] = {0.0, 0.0};
                if (act && tune)
                    for (int e = lt; e < m; e += PG_TR) {
                        const int i = e * PG_RB + lb;
                        const double pv = PV[i], pa = sqrt(pg_abs2(PF[i]));
                        const double dI0 = 0.5 / (wv + pv), tmp = 1.0 / (1.0 + pv / wv);
                        const double q = (YM[i] - pa) * tmp;
                        v[0] += q * q + wv * wv * dI0;
                        v[1] += tmp;
                    }
                pg_red(v, red, t);
                if (act && tune) {
                    wv = (1.0 - 1.0) * wv + 1.0 * (v[0] / v[1]);
                    if (lt == 0) ps[PS_WV][lb] = wv;
                }
                double u[1] = {0.0};
                if (act)
                    for (int e = lt; e < m; e += PG_TR) {
                        const int i = e * PG_RB + lb;
                        const double pv = PV[i], y = YM[i];
                        const d2 pf = PF[i];
                        const double pa = sqrt(pg_abs2(pf)), vv = wv + pv, dy = y - pa;
                        const double ls = log(2.0 * y / vv) - dy * dy / vv + bessel_log_i0e(2.0 * y * pa / vv);
                        u[0] += ls + pg_abs2(csub(AX[i], pf)) / pv;
                    }
                pg_red(u, red, t);
                val = u[0] + ps[PS_VALIN][lb];
            }
            // ---------------- the pass test (gampEst.m:467-471) and the step
            bool pass = false;
            double sf_old = sf;
            if (act) {
                const int cnt = wn < wtry + 1 ? wn : wtry + 1;
                double vmin = win[(wn - 1) & (PG_WIN - 1)][lb];
                for (int k = 2; k <= cnt; ++k) vmin = fmin(vmin, win[(wn - k) & (PG_WIN - 1)][lb]);
                pass = it == 1 || step <= 0.05 || val >= vmin;
                if (pass) {
                    sf = sfsum / a.md;
                    step = fmin(1.1 * fmax(step, 0.05), 0.25);
                    if (lt == 0) {
                        win[wn & (PG_WIN - 1)][lb] = val;
                        ps[PS_VALP][lb] = val;
                        pi[PI_WN][lb] = wn + 1;
                        pi[PI_NPASS][lb] = pi[PI_NPASS][lb] + 1;
                        ps[PS_SF][lb] = sf;
                    }
                } else {
                    step = fmin(fmax(0.05, 0.2 * step), 0.25);
                }
                if (lt == 0) ps[PS_STEP][lb] = step;
            }
            // ---------------- the output estimator, shatNew / svarNew, the damping
            for (int e = lt; e < MP; e += PG_TR) {
                PG_VECS(wsb, nN, nM)
                const int i = e * PG_RB + lb;
                d2 sh = make_double2(0.0, 0.0);
                double sv = 0.0;
                if (act && e < m) {
                    d2 sho, shn;
                    double svo, svn;
                    if (pass) {
                        sho = SH[i];
                        svo = SV[i];
                        const double pv = PV[i], pvr = fmax(pv, 1e-12);
                        const d2 ph_ = PH[i];
                        d2 zh;
                        double zv;
                        pg_estim(YM[i], ph_, pvr, wv, zh, zv);
                        shn = cscale(csub(zh, ph_), sf / pvr);
                        svn = (sf / pvr) * (1.0 - fmin(zv / pvr, INFINITY));
                        if (first_cold) svo = svn;   // svar0 missing: "equivalent to making step=1"
                        PVO[i] = pv;
                        AXF[i] = AX[i];
                        SHO[i] = sho;
                        SVO[i] = svo;
                        SHN[i] = shn;
                        SVN[i] = svn;
                    } else {
                        sho = SHO[i];
                        svo = SVO[i];
                        shn = SHN[i];
                        svn = SVN[i];
                    }
                    sh = cadd(cscale(sho, 1.0 - step), cscale(shn, step));
                    sv = (1.0 - step) * svo + step * svn;
                    if (fabs(sv) < PG_EPS) sv = PG_EPS;
                    SH[i] = sh;
                    SV[i] = sv;
                }
                shL[lb * ST + e] = sh;
                svL[lb * ST + e] = sv;
            }
            // ---------------- N-space before the sweep: the Opt copies, the exports, the tolerance sums, xhatDamp
            {
                PG_VECS(wsb, nN, nM)
                double v[2] = {0.0, 0.0};
                if (act)
                    for (int j = lt; j < N; j += PG_TR) {
                        const size_t i = (size_t)j * PG_RB + lb;
                        d2 xo, xdo;
                        if (pass) {
                            const d2 prev = XO[i];
                            xo = XH[i];
                            if (it > 1) {
                                v[0] += pg_abs2(csub(prev, xo));
                                v[1] += pg_abs2(xo);
                            }
                            xdo = first_cold ? xo : XD[i];   // xhatPrev0 missing: "equivalent to making step=1"
                            XO[i] = xo;
                            XDO[i] = xdo;
                            RHF[i] = it == 1 ? make_double2(NAN, NAN) : RH[i];
                            RVF[i] = it == 1 ? NAN : RV[i] * sf_old;
                        } else {
                            xo = XO[i];
                            xdo = XDO[i];
                        }
                        XD[i] = cadd(cscale(xdo, 1.0 - step), cscale(xo, step));
                    }
                pg_red(v, red, t);   // (its barriers also order the operand stores before the sweep's loads)
                if (act && pass && it > 1 && !stopnow && v[0] / v[1] < ps[PS_TOL2][lb]) stopnow = true;
            }

            // ---------------- backward sweep: D^H shat, |D|^2^T svar, raw sums to RH / RV
            asm volatile("" : "+v"(ln));
            int wb = w;
            asm volatile("" : "+s"(wb));
            lb = ln & 15;
            const int frw = (ln & 15) * ST + (ln >> 4);
            for (int tp = wb; tp < npair; tp += PG_WAVES) {
                PG_VECS(wsb, nN, nM)
                const int j0 = tp * (16 * PG_TW);
                d2 fa[PG_TW][PG_SK], fb[PG_TW][PG_SK];
                d4v cr[PG_TW], ci4[PG_TW], re[PG_TW];
#pragma unroll
                for (int c = 0; c < PG_TW; ++c) cr[c] = ci4[c] = re[c] = d4v{0.0, 0.0, 0.0, 0.0};
                auto gload = [&](d2(&f)[PG_TW][PG_SK], int s) {
#pragma unroll
                    for (int kk = 0; kk < PG_SK; ++kk) {
                        const int e = 4 * (PG_SK * s + kk) + (ln >> 4);
#pragma unroll
                        for (int c = 0; c < PG_TW; ++c) {
                            const int j = j0 + 16 * c + (ln & 15);
                            f[c][kk] = make_double2(0.0, 0.0);
                            if (e < m && j < N) f[c][kk] = D[(size_t)e * N + j];
                        }
                    }
                };
                auto comp = [&](const d2(&f)[PG_TW][PG_SK], int s) {
#pragma unroll
                    for (int kk = 0; kk < PG_SK; ++kk) {
                        const d2 r = shL[frw + 4 * (PG_SK * s + kk)];
                        const double rv = svL[frw + 4 * (PG_SK * s + kk)];
#pragma unroll
                        for (int c = 0; c < PG_TW; ++c) {
                            const d2 v = f[c][kk];
                            cmma(cr[c], ci4[c], make_double2(v.x, -v.y), r);   // applied conjugated
                            re[c] = mfma64(v.x * v.x + v.y * v.y, rv, re[c]);
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
                // lane l, register q: atom j0 + 16 c + (l >> 4) + 4 q, realisation l & 15
                if (act) {
#pragma unroll 1
                    for (int cq = 0; cq < 4 * PG_TW; ++cq) {
                        const int j = j0 + 16 * (cq >> 2) + (ln >> 4) + 4 * (cq & 3);
                        const double acr = pg_pick(cr, cq), aci = pg_pick(ci4, cq), are = pg_pick(re, cq);
                        if (j < N) {
                            RH[(size_t)j * PG_RB + lb] = make_double2(acr, aci);
                            RV[(size_t)j * PG_RB + lb] = are;
                        }
                    }
                }
            }
            __syncthreads();

            // ---------------- N-space after the sweep: rvar, rhat, SparseScaEstim around CAwgnEstimIn
            asm volatile("" : "+v"(ln));
            lb = ln & 15, lt = 4 * w + (ln >> 4);
            bool raised = false;
            {
                PG_VECS(wsb, nN, nM)
                double p1 = ps[PS_P1][lb], vx = ps[PS_VX][lb];
                const double sf = ps[PS_SF][lb];
                const double lpr = log(1.0 - p1) - log(p1);
                double v[1] = {0.0};
                if (act)
                    for (int j = lt; j < N; j += PG_TR) {
                        const size_t i = (size_t)j * PG_RB + lb;
                        const d2 raw = RH[i];
                        const double rvar = 1.0 / RV[i];
                        const d2 rhat = cadd(XD[i], cscale(raw, rvar));
                        RH[i] = rhat;
                        RV[i] = rvar;
                        const double rvs = fmax(rvar, 1e-12) * sf;
                        const double r2 = pg_abs2(rhat);
                        const double ll1 = -(log(M_PI) + log(vx + rvs) + r2 / (vx + rvs));
                        const double rv = rvs < PG_EPS ? PG_EPS : rvs;
                        const double ll0 = -(log(M_PI) + log(rv) + r2 / rv);
                        const double ex = fmax(fmin(ll0 - ll1 + lpr, 500.0), -500.0);
                        const double py1 = 1.0 / (1.0 + exp(ex));
                        PY[i] = py1;
                        v[0] += py1;
                    }
                pg_red(v, red, t);
                if (act && tune) p1 = v[0] / a.Nd;
                const double lp1 = fmax(1e-8, p1), lp0 = fmax(1e-8, 1.0 - p1);
                double u[2] = {0.0, 0.0};
                if (act)
                    for (int j = lt; j < N; j += PG_TR) {
                        const size_t i = (size_t)j * PG_RB + lb;
                        const d2 rhat = RH[i];
                        const double rvs = fmax(RV[i], 1e-12) * sf;
                        const double rv = rvs < PG_EPS ? PG_EPS : rvs;
                        const double py1 = PY[i], py0 = 1.0 - py1;
                        const double gain = vx / (vx + rv);
                        const d2 xh1 = cscale(rhat, gain);
                        const double xv1 = gain * rv, xr = rv / (vx + rv);
                        const double q1 = pg_abs2(xh1);
                        u[0] += (py1 / p1) * q1 + xv1;
                        const double v1 = log(xr) + (1.0 - xr) - q1 / vx;
                        const d2 xh = cscale(xh1, py1);
                        const double q = pg_abs2(xh);
                        XH[i] = xh;
                        XV[i] = py1 * (q1 - q) + py1 * xv1 + py0 * (0.0 - q);
                        u[1] += py1 * v1 + py1 * log(lp1 / fmax(py1, 1e-8)) + py0 * log(lp0 / fmax(py0, 1e-8));
                    }
                pg_red(u, red, t);   // (its barriers also order these stores before the next sweep's loads)
                if (act) {
                    if (lt == 0) ps[PS_VALIN][lb] = u[1];
                    if (tune) {
                        const double nv = u[0] / a.Nd;
                        if (!(nv > 0.0)) raised = true;   // CAwgnEstimIn.set.var0's assert
                        if (lt == 0) {
                            ps[PS_P1][lb] = p1;
                            ps[PS_VX][lb] = fmax(PG_EPS, nv);
                        }
                    }
                }
            }
            if (act) {
                gstop = stopnow;
                if (raised) {
                    stat |= ACE_ST_PRGAMP_FAILED;
                    fl |= F_RAISED | F_DONE;
                    gstop = true;
                }
            }
        }

        // ================================================= after the call (prGAMP4.m:681-747, :749-901)
        int pl = t;
        asm volatile("" : "+v"(pl));
        const int pb = pl & 15, pt = pl >> 4;   // = bc, tr (opaque, as above)
        const long long pbb = (long long)blockIdx.x * PG_RB + pb;
        PG_VECS(wsb, nN, nM)
        const bool fin = incall && !(fl & F_DONE);   // (done here: the tuning raised)
        if (fin && pt == 0) {
            const size_t slot = ((size_t)pbb * a.max_try + (ntry - 1)) * (a.nit_em + 1) + em;
            if (a.trace) {
                a.trace[slot * 2] = it;
                a.trace[slot * 2 + 1] = pi[PI_NPASS][pb];
            }
            if (a.vals) a.vals[slot] = ps[PS_VALP][pb];
        }
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (fin) {
            for (int e = pt; e < m; e += PG_TR) {
                const double q = sqrt(pg_abs2(AXF[e * PG_RB + pb])) - YM[e * PG_RB + pb];
                v[0] += q * q;
            }
            for (int j = pt; j < N; j += PG_TR) {
                const size_t i = (size_t)j * PG_RB + pb;
                const d2 xo = XO[i];
                v[1] += pg_abs2(RHF[i]);
                v[2] += em > 0 ? pg_abs2(csub(XP[i], xo)) : 0.0;
                v[3] += pg_abs2(xo);
            }
        }
        pg_red(v, red, t);
        bool endtry = false, take = false, final_stop = false;
        double nres = NAN;
        const double wv_start = ps[PS_WVS][pb];
        const double snrhat = 10.0 * log10(ps[PS_MY2][pb] / wv_start);
        const double tolem = 10.0 * fmin(pow(10.0, -snrhat / 10.0), 1e-4);
        if (fin) {
            const double xvar0 = ps[PS_XVAR0][pb];
            nres = 20.0 * log10(sqrt(v[0]) / sqrt(ps[PS_NY2][pb]));
            const bool nonzero = v[1] > 1e-6 * a.sr * (a.Nd * xvar0);
            if (pt == 0) {
                ps[PS_LP1][pb] = ps[PS_P1][pb];
                ps[PS_LVX][pb] = ps[PS_VX][pb];
            }
            if (isnan(nres) || isinf(nres) || !nonzero) {
                if (pt == 0) {
                    ps[PS_GAIN][pb] = ps[PS_GAIN][pb] * 2.0;
                    pi[PI_WINDOW][pb] = (3 * pi[PI_WINDOW][pb] + 3) / 4;   // ceil(0.75 stepWindow)
                }
                endtry = true;
            } else {
                const double q = em > 0 ? sqrt(v[2]) / sqrt(v[3]) : INFINITY;
                if (q < tolem || em == a.nit_em) endtry = true;
            }
            if (endtry) {
                const double best = ps[PS_BEST][pb];
                take = nres < best;
                const double nbest = take ? nres : best;
                final_stop = nbest < a.stopdb;
            } else {
                // GampOpt.warmStart: shatNext = shat / scaleFac, then shat0 scaleFac (gampEst.m:658, :254)
                for (int j = pt; j < N; j += PG_TR) XP[(size_t)j * PG_RB + pb] = XO[(size_t)j * PG_RB + pb];
                const double sf = ps[PS_SF][pb];
                for (int e = pt; e < m; e += PG_TR) {
                    const int i = e * PG_RB + pb;
                    SH[i] = cscale(cscale(SH[i], 1.0 / sf), sf);
                    SV[i] = (SV[i] / sf) * sf;
                }
                ++em;
                fl &= ~F_COLD;
            }
        }
        __syncthreads();   // (the reads of the try-level scalars above, before the writes below)
        if (take) {
            for (int j = pt; j < N; j += PG_TR) {
                const size_t i = (size_t)j * PG_RB + pb;
                XB[i] = XO[i];
                RHB[i] = RHF[i];
                RVB[i] = RVF[i];
            }
            if (pt == 0) {
                ps[PS_BEST][pb] = nres;
                ps[PS_BWV][pb] = wv_start;
                ps[PS_BSNR][pb] = snrhat;
                pi[PI_BT][pb] = ntry;
                pi[PI_BEM][pb] = em + 1;
                pi[PI_HAVE][pb] = 1;
            }
        }
        double sc[1] = {0.0};
        if (final_stop) {   // the posterior support count (:887-893) on estFin_best (this thread's own stores above)
            const double xvar0 = ps[PS_XVAR0][pb];
            for (int j = pt; j < N; j += PG_TR) {
                const size_t i = (size_t)j * PG_RB + pb;
                const double r2 = pg_abs2(take ? RHF[i] : RHB[i]), rv = take ? RVF[i] : RVB[i];
                const double pp = 1.0 / (1.0 + a.odds * exp(-r2 / rv + r2 / (rv + xvar0)) * (rv + xvar0) / rv);
                if (pp > 0.5) sc[0] += 1.0;
            }
        }
        pg_red(sc, red, t);
        if (final_stop) {
            if (pt == 0) pi[PI_SUPP][pb] = (int)sc[0];
            fl |= F_STOPPED | F_DONE;
        } else if (endtry) {
            fl |= ntry >= a.max_try ? F_DONE : F_NEWTRY;
        }
        __syncthreads();
    }

    // ---------------- outputs
    if (!live) return;
    int ol = t;
    asm volatile("" : "+v"(ol));
    const int ob = ol & 15, ot = ol >> 4;
    const long long obb = (long long)blockIdx.x * PG_RB + ob;
    PG_VECS(wsb, nN, nM)
    const bool have = pi[PI_HAVE][ob] != 0;
    if (!(stat & (ACE_ST_EVAL_DEGENERATE | ACE_ST_PRGAMP_FAILED))) {
        if (!have) stat |= ACE_ST_PRGAMP_FAILED;   // prGAMP4.m:909: estFin_best was never assigned
        else if (!(fl & F_STOPPED)) stat |= ACE_ST_PRGAMP_MAXTRY;
    }
    const bool ok = have && !(stat & ACE_ST_PRGAMP_FAILED);
    for (int j = ot; j < N; j += PG_TR)
        a.xhat[(size_t)obb * N + j] = ok ? XB[(size_t)j * PG_RB + ob] : make_double2(0.0, 0.0);
    if (ot == 0) {
        double* const o = a.info + obb * 8;
        o[0] = ok ? ps[PS_BEST][ob] : 0.0;
        o[1] = ok ? ps[PS_BWV][ob] : 0.0;
        o[2] = ok ? ps[PS_LP1][ob] : 0.0;
        o[3] = ok ? ps[PS_LVX][ob] : 0.0;
        o[4] = 0.0;   // xmean0sq_hat: mean0 is 0 and not tuned
        o[5] = ok ? ps[PS_BSNR][ob] : 0.0;
        o[6] = o[7] = 0.0;
        int32_t* const c = a.counts + obb * 4;
        c[0] = (fl & F_RAISED) ? 0 : ntry;   // numTry (a raise leaves nothing behind)
        c[1] = ok ? pi[PI_BT][ob] : 0;
        c[2] = ok ? pi[PI_BEM][ob] : 0;
        c[3] = ok ? pi[PI_SUPP][ob] : -1;
        if (a.status) a.status[obb] = stat;
    }
}

int pg_check_args(const ace_prgamp_cfg* cfg, int batch, int m, int N, const double* D, const double* Y, const double* G,
                  const double* xhat, const double* info, const int32_t* counts) {
    if (!cfg) return fail(ACE_ERR_ARG, "prgamp: NULL cfg");
    if (batch < 1) return fail(ACE_ERR_ARG, "prgamp: batch %d < 1", batch);
    if (m < 1 || m > PG_MMAX) return fail(m < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "prgamp: m %d outside 1..%d", m, PG_MMAX);
    if (N < 1 || N > PG_NMAX) return fail(N < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "prgamp: N %d outside 1..%d", N, PG_NMAX);
    if (!(cfg->sparse_rat > 0.0 && cfg->sparse_rat <= 1.0))
        return fail(ACE_ERR_ARG, "prgamp: sparse_rat %g outside (0, 1]", cfg->sparse_rat);
    if (!std::isfinite(cfg->snr_db) || !std::isfinite(cfg->snr_db_init))
        return fail(ACE_ERR_ARG, "prgamp: snr_db / snr_db_init is not finite");
    if (cfg->max_try < 1) return fail(ACE_ERR_ARG, "prgamp: max_try %d < 1", cfg->max_try);
    if (cfg->nit_em < 0) return fail(ACE_ERR_ARG, "prgamp: nit_em %d < 0", cfg->nit_em);
    if (cfg->gamp_nit < 1) return fail(ACE_ERR_ARG, "prgamp: gamp_nit %d < 1", cfg->gamp_nit);
    if (!D || !Y || !G || !xhat || !info || !counts)
        return fail(ACE_ERR_ARG, "prgamp: NULL %s", !D ? "D" : !Y ? "Y" : !G ? "G" : !xhat ? "xhat" : !info ? "info" : "counts");
    return ACE_OK;
}

size_t pg_ws_bytes(int batch, int m, int N) {
    const size_t ng = ((size_t)batch + PG_RB - 1) / PG_RB;
    return ((ng * pg_group_doubles(m, N) * sizeof(double) + 255) & ~(size_t)255) + 256;   // (the base is rounded up to 256 B)
}

}  // namespace

size_t prgamp_request_bytes(int m) { return pg_lds_bytes(m < 1 ? 1 : m > PG_MMAX ? PG_MMAX : m); }

}  // namespace ace

using namespace ace;

extern "C" void ace_prgamp_cfg_default(ace_prgamp_cfg* cfg) {
    if (!cfg) return;
    cfg->sparse_rat = 0.0;   // s / n: the caller's
    cfg->snr_db_init = 20.0;
    cfg->snr_db = 25.0;
    cfg->max_try = 100;
    cfg->nit_em = 50;
    cfg->gamp_nit = 200;
    cfg->reserved = 0;
}

extern "C" size_t ace_prgamp_workspace_size(int batch, int m, int N, int max_try) {
    if (batch < 1 || m < 1 || m > PG_MMAX || N < 1 || N > PG_NMAX || max_try < 1) return 0;
    return pg_ws_bytes(batch, m, N);
}

extern "C" int ace_prgamp_solve_batch(const ace_prgamp_cfg* cfg, int batch, int m, int N, const double* D, const double* Y,
                                      const double* G, double* xhat, double* info, int32_t* counts, uint32_t* status,
                                      int32_t* trace, double* vals, void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(pg_check_args(cfg, batch, m, N, D, Y, G, xhat, info, counts));
    const size_t need = pg_ws_bytes(batch, m, N);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "prgamp: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    // 96 KiB of dynamic LDS and more, past the 64 KiB default: the kernel's derived budget decides (no fallback)
    const void* const kern = reinterpret_cast<const void*>(&prgamp_kernel);
    const size_t lds = pg_lds_bytes(m);
    if (!lds_ok(kern, lds))
        return fail(ACE_ERR_UNSUPPORTED, "prgamp: prgamp_kernel needs %zu B of dynamic LDS, budget %zu B", lds, lds_dyn_budget(kern));
    PrGampArgs a;
    a.batch = batch;
    a.m = m;
    a.N = N;
    a.max_try = cfg->max_try;
    a.nit_em = cfg->nit_em;
    a.nit = cfg->gamp_nit;
    a.sr = std::fmin(cfg->sparse_rat, 0.9);
    const double snrdb = std::fmin(100.0, cfg->snr_db);
    a.snr = std::pow(10.0, snrdb / 10.0);
    a.snri = std::pow(10.0, std::fmin(100.0, cfg->snr_db_init) / 10.0);
    a.stopdb = -(snrdb + 2.0);
    a.odds = (1.0 - a.sr) / a.sr;
    a.Nd = N;
    a.md = m;
    a.D = (const d2*)D;
    a.Y = Y;
    a.G = (const d2*)G;
    a.xhat = (d2*)xhat;
    a.info = info;
    a.counts = counts;
    a.status = status;
    a.trace = trace;
    a.vals = vals;
    a.ws = (double*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    // the slots of calls that never run read 0
    const size_t nslot = (size_t)batch * cfg->max_try * ((size_t)cfg->nit_em + 1);
    if (trace) ACE_HIP(hipMemsetAsync(trace, 0, nslot * 2 * sizeof(int32_t), (hipStream_t)stream));
    if (vals) ACE_HIP(hipMemsetAsync(vals, 0, nslot * sizeof(double), (hipStream_t)stream));
    const int nblk = (batch + PG_RB - 1) / PG_RB;
    hipLaunchKernelGGL(prgamp_kernel, dim3(nblk), dim3(PG_NT), lds, (hipStream_t)stream, a);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_prgamp_solve_host(const ace_prgamp_cfg* cfg, int batch, int m, int N, const double* D, const double* Y,
                                     const double* G, double* xhat, double* info, int32_t* counts, uint32_t* status,
                                     int32_t* trace, double* vals) {
    g_err.clear();
    ACE_TRY(pg_check_args(cfg, batch, m, N, D, Y, G, xhat, info, counts));
    const size_t B = batch, wsb = pg_ws_bytes(batch, m, N), nslot = B * cfg->max_try * ((size_t)cfg->nit_em + 1);
    DevScope dev;
    double *dD, *dY, *dG, *dxhat, *dinfo, *dvals = nullptr;
    int32_t *dcnt, *dtr = nullptr;
    uint32_t* dst = nullptr;
    char* dws;
    ACE_TRY(dev.put(&dD, D, 2 * (size_t)m * N));
    ACE_TRY(dev.put(&dY, Y, B * m));
    ACE_TRY(dev.put(&dG, G, 2 * B * cfg->max_try * N));
    ACE_TRY(dev.alloc(&dxhat, 2 * B * N));
    ACE_TRY(dev.alloc(&dinfo, 8 * B));
    ACE_TRY(dev.alloc(&dcnt, 4 * B));
    if (status) ACE_TRY(dev.alloc(&dst, B));
    if (trace) ACE_TRY(dev.alloc(&dtr, 2 * nslot));
    if (vals) ACE_TRY(dev.alloc(&dvals, nslot));
    ACE_TRY(dev.alloc(&dws, wsb));
    ACE_TRY(ace_prgamp_solve_batch(cfg, batch, m, N, dD, dY, dG, dxhat, dinfo, dcnt, dst, dtr, dvals, dws, wsb, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(xhat, dxhat, 2 * B * N));
    ACE_TRY(dev.get(info, dinfo, 8 * B));
    ACE_TRY(dev.get(counts, dcnt, 4 * B));
    ACE_TRY(dev.get(trace, dtr, 2 * nslot));
    ACE_TRY(dev.get(vals, dvals, nslot));
    return dev.get(status, dst, B);
}
