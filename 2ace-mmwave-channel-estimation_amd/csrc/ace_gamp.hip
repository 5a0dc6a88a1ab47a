// Batched complex EM-BG-GAMP against one shared dictionary D [d][N]: the second stage of the two-stage PLGAMP
// recovery (My_TwoStage_Recovery.m:163-181) and the first branch of My_Conventional_CS.m:79.  The reference vendors
// the solver (3rd_software_component/GAMP/trunk/code: EMGMAMP/EMBGAMP.m -> EMGMAMP/EMGMAMP.m, main/gampEst.m,
// CAwgnEstimIn, CAwgnEstimOut, SparseScaEstim, EMGMAMP/CBG_update.m, set_initsBG.m, check_opts.m, EMOpt.m); this
// restates what those files do for the two option sets of include/ace.h, T = 1 column per realisation.
//
// One kernel, one launch: every EM iteration, every GAMP iteration inside it and the final GAMP call.  A
// work-group (8 waves) owns GA_RB = 16 realisations, the columns of one MFMA tile, and runs them to the end.  A
// realisation that has stopped (its GAMP call, or everything) idles with its state frozen: its column of the
// products is still computed and then dropped, nothing of it is written.  The group leaves a GAMP call when all
// of its realisations have stopped it, and the kernel when all are done.  All control state is per realisation
// (step, the last passed utility, valIn, stop flags, counters, lambda / phi / psi; gampEst's fail count is not
// kept: with maxBadSteps = inf nothing reads it): thread t serves
// realisation t & 15 in every phase, and the 32 threads of a realisation hold identical copies of its control
// state, computed from the same reduced sums.  Nothing is combined across work-groups; there are no atomics.
//
// A GAMP iteration (gampEst.m:403-653 with scaleFac = 1, no pvar / rvar steps, pvarMin = xvarMin = 0):
//   forward sweep   Axhat = D xhat (complex) and A2xvar = |D|^2 xvar (real) on v_mfma_f64_16x16x4_f64 (cmma / mfma64
//                   of ace_mfma.hpp).  The complex product is the 4M form: the results feed the estimate, and in
//                   the 4M form each of Re, Im is an ordinary real dot product of 2 N terms, so an entry errs by at
//                   most gamma_{2N} sum_j |d_ej| |x_j| (componentwise), which the 3M form does not give for the
//                   imaginary part.  |D|^2 is formed from the fragment already in registers (one multiply-add; no
//                   second matrix is read or stored).  D is the A operand (rows e), xhat / xvar the B operand (the
//                   16 realisations), the k index runs over atoms.  The sum over N is split across the waves (wave
//                   w takes the 16-atom chunks w, w + 8, ...), 32 rows of D at a time; the eight partial tiles go to
//                   LDS and thread (row, realisation) adds them in wave order 0 .. 7.
//   m-space step    d entries x 16 realisations, entry e on thread (e & 31, realisation): phat, the utility
//                   val = sum logLike + valIn (reduced in a fixed order), the pass test (forced on the first
//                   iteration of a call), zhat / zvar, shatNew / svarNew, the step update and the damping; the
//                   damped shat / svar go to LDS as the B operand of the backward sweep, |svar| < eps becomes eps.
//   backward sweep  D^H shat and |D|^2^T svar, the structure of omp_kernel's correlation step (a wave walks pairs
//                   of 16-atom tiles, D^H fragments straight from global memory, two register sets).  Epilogue per
//                   atom: on a passed step the "Opt" copies and the exports (xhatOpt = xhatFinal, xvarFinal,
//                   xhatDampOpt, rhatFinal, rvarFinal) and the sums of the tolerance test; then xhatDamp, rvar, rhat,
//                   SparseScaEstim around CAwgnEstimIn (activity posterior with the exponent clipped to +-500,
//                   xhat, xvar, the negative KL term; rvar floored at eps except inside loglike1, as the reference
//                   has it).  valIn and the tolerance sums are reduced in a fixed order.
// The N-long vectors (xhat, xvar, xhatDamp, rhat, rvar, their "Opt" / "Final" copies, XhatPrev of the EM loop) and
// the d-long ones live in the caller's workspace, [index][16 realisations] per work-group: 144 B per atom and
// 112 B per row and realisation.  They do not fit LDS.
//
// EM (EMGMAMP.m:277-411 with L = 1, heavy_tailed, maxBethe, joint noise, per-column signal parameters): after
// each GAMP call CBG_update for phi (and lambda when learned; A_n NaN becomes 0.999), phi >= minVar = 1e-5,
// psi <- psi sum |shat|^2 / sum svar, EMtol = min(0.1 psi / ||y||, 1e-4) and the stopping test.  The warm start of
// GampOpt.warmStart after a completed EM iteration is "leave everything where it is": xhatNext, xvarNext, shatNext,
// svarNext, xhatDamp, valIn, the last passed utility (stepWindow = 0: only the last one is ever compared) and step
// stay in place, although psi, phi and lambda have changed under them.  rhat / rvar / zhat / zvar of a call exist
// from its second pass on: a call with one pass leaves the EM loop (EMGMAMP.m:320) BEFORE its warm start is taken
// (:400), so the final call runs from the entry state of the call that broke (restored from the Opt copies and three
// saved scalars), after the post-loop update has scaled psi by the last ratio once more (it does so after every exit).
//
// What raises in the reference, and so sets ACE_ST_GAMP_FAILED (xhat zeroed; the caller's catch runs OMP):
//   - CAwgnEstimOut's assert(all(wvar >= 0)): psi NaN or negative, before any call;
//   - CAwgnEstimIn's assert(all(var0 > 0)): the initial phi of set_initsBG is 0 (y = 0), NaN (||y||^2 overflows) or
//     negative; later values are floored at minVar (MATLAB's max(NaN, 1e-5) is 1e-5);
//   - the NaN break in the first EM iteration: the post-loop update reads Shat, which was never assigned.
//
// Batch invariance: a realisation's outputs are a function of (y_b, D, cfg, d, N) alone.  Its column of every MFMA
// result does not depend on the other columns, the chunk and tile walks depend on N and d only, every sum has a
// fixed order (per-thread in index order, then 32 partials in thread order, the waves' tiles in wave order).
//
// LDS: dynamic max(8 x 32 x 16 x 3 doubles of forward partials, 16 (DP + 1) x 24 B of shat / svar) = 98304 B up to
// d = 240 and 98688 B at d = 256 (DP = 16 ceil(d / 16)), through the kernel's derived budget (lds_dyn_budget; no
// second path), plus 17152 B static (the reductions and the calls' entry scalars).  240 VGPRs (two waves per SIMD), no
// VGPR spill and no scratch.  That took three things: the wave index as a scalar (readfirstlane), and the lane and
// thread indices, the wave index and the workspace bases behind opaque copies renewed per phase (GA_VECS, the empty
// asm statements), so that the addresses each phase derives from them are formed inside it; left to itself the
// compiler hoists them all in front of the main loop and keeps them, in registers and then in scratch, across every
// phase.  The scalar side still parks 83 values in the lanes of a VGPR (v_writelane / v_readlane, no memory): kernel
// arguments, sizes and loop-invariant masks beyond the 102 scalar registers of a wave.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

#include <cmath>

namespace ace {
namespace {

constexpr int GA_WAVES = 8;
constexpr int GA_NT = 64 * GA_WAVES;
constexpr int GA_RB = 16;               // realisations per work-group (the columns of one MFMA tile)
constexpr int GA_TR = GA_NT / GA_RB;    // threads of a realisation
constexpr int GA_DMAX = 256;
constexpr int GA_NMAX = 16384;
constexpr int GA_RT = 2;                // row tiles of the forward sweep per pass (32 rows)
constexpr int GA_TW = 2;                // atom tiles per wave and pass of the backward sweep
constexpr int GA_SK = 4;                // k-steps per chunk
constexpr int GA_NITMAX = 31;           // the pass mask is one int32
constexpr int GA_RK = 4;                // sums per reduction
constexpr double GA_EPS = 0x1p-52;
static_assert(GA_TR == 32 && GA_RT * 16 == GA_TR, "thread layout");

struct GampArgs {
    int batch, d, N, max_em, nit, learn;
    double snr_lin;   // 1 + 10^(min(100, SNRdB) / 10)
    double lam0, step0, tol;
    const d2* D;
    const d2* Y;
    d2* xhat;
    double* xvar;
    double* params;
    int32_t* em_iters;
    int32_t* trace;
    uint32_t* status;
    double* ws;
};

constexpr size_t ga_lds_bytes(int d) {
    const size_t part = (size_t)GA_WAVES * GA_TR * GA_RB * 3 * sizeof(double);
    const size_t opnd = (size_t)GA_RB * ((d + 15) / 16 * 16 + 1) * (sizeof(d2) + sizeof(double));
    return part > opnd ? part : opnd;
}
// workspace of a work-group in doubles: 7 complex + 4 real N-vectors, 5 complex + 4 real d-vectors, [index][16]
constexpr size_t ga_group_doubles(int d, int N) {
    return (size_t)18 * N * GA_RB + (size_t)14 * ((d + 15) / 16 * 16) * GA_RB;
}

// |a|^2 in one fixed form, fma(re, re, im im): left to the compiler's contraction, two instances of
// re re + im im may be fused differently (fma(re, re, im im) here, fma(im, im, re re) there) and then differ by an
// ulp on the same input
__device__ __forceinline__ double ga_abs2_rn(d2 a) {
    const double yy = a.y * a.y;
    return __builtin_fma(a.x, a.x, yy);
}

// element cq = 4 c + q of the GA_TW accumulators, by selects (no dynamic register index)
__device__ __forceinline__ double ga_pick(const d4v (&v)[GA_TW], int cq) {
    double r = v[0][0];
#pragma unroll
    for (int c = 0; c < GA_TW; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) r = cq == 4 * c + q ? v[c][q] : r;
    return r;
}

// v[k] <- the sum over the 32 threads of the realisation, in thread order: the same bits in all of them
template <int K>
__device__ __forceinline__ void ga_red(double (&v)[K], double* red, int t) {
    static_assert(K <= GA_RK, "reduction buffer");
#pragma unroll
    for (int k = 0; k < K; ++k) red[(k * GA_TR + (t >> 4)) * GA_RB + (t & 15)] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < GA_TR; ++i) s += red[(k * GA_TR + i) * GA_RB + (t & 15)];
        v[k] = s;
    }
    __syncthreads();
}

// The vectors of the work-group's workspace, declared where a phase uses them, from a copy of the base that the compiler
// cannot see through: the twenty bases are then formed inside the phase and do not occupy scalar registers (or the lanes
// they would be spilled to) across the others.  nN_ = 16 N, nM_ = 16 DP doubles per real vector.
#define GA_VECS(wsb_, nN_, nM_) \
    double* gq_ = (wsb_); \
    size_t gn_ = (nN_), gm_ = (nM_); \
    asm volatile("" : "+s"(gq_), "+s"(gn_), "+s"(gm_)); \
    [[maybe_unused]] d2* const XH = (d2*)(gq_ + 0 * gn_ + 0 * gm_); /* xhat */ \
    [[maybe_unused]] d2* const XD = (d2*)(gq_ + 2 * gn_ + 0 * gm_); /* xhatDamp */ \
    [[maybe_unused]] d2* const XO = (d2*)(gq_ + 4 * gn_ + 0 * gm_); /* xhatOpt = xhatFinal */ \
    [[maybe_unused]] d2* const XDO = (d2*)(gq_ + 6 * gn_ + 0 * gm_); /* xhatDampOpt */ \
    [[maybe_unused]] d2* const RH = (d2*)(gq_ + 8 * gn_ + 0 * gm_); /* rhat */ \
    [[maybe_unused]] d2* const RHF = (d2*)(gq_ + 10 * gn_ + 0 * gm_); /* rhatFinal */ \
    [[maybe_unused]] d2* const XP = (d2*)(gq_ + 12 * gn_ + 0 * gm_); /* XhatPrev of the EM loop */ \
    [[maybe_unused]] double* const XV = (double*)(gq_ + 14 * gn_ + 0 * gm_); /* xvar */ \
    [[maybe_unused]] double* const XVF = (double*)(gq_ + 15 * gn_ + 0 * gm_); /* xvarFinal */ \
    [[maybe_unused]] double* const RV = (double*)(gq_ + 16 * gn_ + 0 * gm_); /* rvar */ \
    [[maybe_unused]] double* const RVF = (double*)(gq_ + 17 * gn_ + 0 * gm_); /* rvarFinal */ \
    [[maybe_unused]] d2* const YM = (d2*)(gq_ + 18 * gn_ + 0 * gm_); /* y */ \
    [[maybe_unused]] d2* const SH = (d2*)(gq_ + 18 * gn_ + 2 * gm_); /* shat */ \
    [[maybe_unused]] d2* const SHO = (d2*)(gq_ + 18 * gn_ + 4 * gm_); /* shatOpt */ \
    [[maybe_unused]] d2* const SHN = (d2*)(gq_ + 18 * gn_ + 6 * gm_); /* shatNew */ \
    [[maybe_unused]] d2* const AX = (d2*)(gq_ + 18 * gn_ + 8 * gm_); /* Axhat */ \
    [[maybe_unused]] double* const SV = (double*)(gq_ + 18 * gn_ + 10 * gm_); /* svar */ \
    [[maybe_unused]] double* const SVO = (double*)(gq_ + 18 * gn_ + 11 * gm_); /* svarOpt */ \
    [[maybe_unused]] double* const SVN = (double*)(gq_ + 18 * gn_ + 12 * gm_); /* svarNew */ \
    [[maybe_unused]] double* const A2 = (double*)(gq_ + 18 * gn_ + 13 * gm_); /* A2xvar */

__global__ __launch_bounds__(GA_NT) void gamp_kernel(const GampArgs a) {
    extern __shared__ __align__(16) unsigned char ga_lds[];   // forward partials | shat, svar operands (ga_lds_bytes)
    __shared__ double red[GA_RK * GA_TR * GA_RB];
    __shared__ double sb[GA_RB];
    __shared__ double ent[3][GA_RB];   // step, valIn, valOpt of each realisation at the entry of its current call
    const int d = a.d, N = a.N;
    const int DP = (d + 15) / 16 * 16, ST = DP + 1;
    double* const part = (double*)ga_lds;
    d2* const shL = (d2*)ga_lds;
    double* const svL = (double*)(shL + GA_RB * ST);
    const d2* __restrict__ const D = a.D;

    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);   // (wave-uniform, and said so: a scalar)
    const int bc = t & 15, tr = t >> 4;               // the realisation's column, the thread within it
    const long long b = (long long)blockIdx.x * GA_RB + bc;
    const bool live = b < a.batch;

    // the group's workspace (GA_VECS declares its vectors where they are used)
    const size_t nN = (size_t)N * GA_RB, nM = (size_t)DP * GA_RB;
    double* const wsb = a.ws + (size_t)blockIdx.x * ga_group_doubles(d, N);

    // ---------------- sum |D|^2 (set_initsBG: sum(A.multSqTr(ones))), y, ||y||^2
    double dsum;
    {
        double v[1] = {0.0};
        for (size_t i = t; i < (size_t)d * N; i += GA_NT) v[0] += cabs2(D[i]);
        ga_red(v, red, t);
        if (tr == 0) sb[bc] = v[0];
        __syncthreads();
        dsum = 0.0;
        for (int i = 0; i < GA_RB; ++i) dsum += sb[i];
    }
    double ny2;
    bool bad;
    {
        double v[2] = {0.0, 0.0};
        GA_VECS(wsb, nN, nM)
        for (int e = tr; e < DP; e += GA_TR) {
            d2 y = make_double2(0.0, 0.0);
            if (live && e < d) y = a.Y[(size_t)b * d + e];
            if (!isfinite(y.x) || !isfinite(y.y)) v[1] += 1.0;
            v[0] += cabs2(y);
            YM[e * GA_RB + bc] = y;
            SH[e * GA_RB + bc] = make_double2(0.0, 0.0);
            SV[e * GA_RB + bc] = 0.0;
        }
        ga_red(v, red, t);
        ny2 = v[0];
        bad = v[1] != 0.0;
    }
    // set_initsBG
    double psi = ny2 / (d * a.snr_lin);
    if (psi == 0.0) psi = ny2 / (d * 1e10);
    double lam = a.lam0;
    double phi = (ny2 - d * psi) / dsum / lam;
    uint32_t stat = 0u;
    if (bad) stat = ACE_ST_EVAL_DEGENERATE;
    else if (!(phi > 0.0) || !(psi >= 0.0)) stat = ACE_ST_GAMP_FAILED;
    // cold start of gampEst: xhat = 0, xvar = lambda var0 (SparseScaEstim.estimInit), shat = 0
    {
        const double xv0 = lam * fmax(GA_EPS, phi);
        GA_VECS(wsb, nN, nM)
        for (int j = tr; j < N; j += GA_TR) {
            XH[(size_t)j * GA_RB + bc] = make_double2(0.0, 0.0);
            XV[(size_t)j * GA_RB + bc] = xv0;
        }
    }

    int ph = (!live || stat) ? 2 : (a.max_em < 1 ? 1 : 0);   // 0: in the EM loop, 1: the final call, 2: done
    int t_em = 0, ci = 0;
    bool emstop = false, have_ratio = false, cold = true, ok_out = false;
    double ratio = 1.0, step = a.step0, valIn = -INFINITY, valOpt = -INFINITY;
    const double tol2 = a.tol * a.tol;
    const int nch = (N + 15) / 16, nrg = (d + GA_TR - 1) / GA_TR;
    const int ntile = nch, npair = (ntile + GA_TW - 1) / GA_TW, nst = DP / (4 * GA_SK);

    while (true) {
        if (__syncthreads_or(ph != 2) == 0) break;
        // ================================================= one gampEst call for the realisations with ph < 2
        const bool incall = ph < 2;
        if (ph == 0) {
            ++t_em;
            emstop = t_em >= a.max_em;
        }
        int it = 0, mask = 0, npass = 0;
        bool gstop = !incall;
        if (tr == 0) {   // (read back after the call, many barriers later)
            ent[0][bc] = step;
            ent[1][bc] = valIn;
            ent[2][bc] = valOpt;
        }
        const double wpos = fmax(1e-20, psi);
        while (true) {
            if (__syncthreads_or(!gstop) == 0) break;
            const bool act = !gstop;
            bool stopnow = false;
            if (act) {
                ++it;
                stopnow = it >= a.nit;
            }

            // (the lane index behind an opaque copy, renewed before each phase: indices derived from it are formed inside
            // the phase and do not sit in registers, or in scratch, across the others)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            int lb = ln & 15, lt = 4 * w + (ln >> 4);   // = bc, tr
            int wf = w;   // (the wave index too: what is derived from it is formed inside the sweep)
            asm volatile("" : "+s"(wf));
            // ---------------- forward sweep: Axhat = D xhat, A2xvar = |D|^2 xvar
            for (int rg = 0; rg < nrg; ++rg) {
                GA_VECS(wsb, nN, nM)
                struct FSet {
                    d2 dd[GA_RT][GA_SK];
                };
                d4v cr[GA_RT], ci4[GA_RT], re[GA_RT];
#pragma unroll
                for (int c = 0; c < GA_RT; ++c) cr[c] = ci4[c] = re[c] = d4v{0.0, 0.0, 0.0, 0.0};
                auto fload = [&](FSet& f, int ch) {
#pragma unroll
                    for (int kk = 0; kk < GA_SK; ++kk) {
                        const int j = 16 * ch + 4 * kk + (ln >> 4);
                        const bool in = j < N;
#pragma unroll
                        for (int c = 0; c < GA_RT; ++c) {
                            const int e = GA_TR * rg + 16 * c + (ln & 15);
                            f.dd[c][kk] = make_double2(0.0, 0.0);
                            if (in && e < d) f.dd[c][kk] = D[(size_t)e * N + j];
                        }
                    }
                };
                // (xhat / xvar: 256 contiguous bytes per k-step, read where they are used; only D is prefetched)
                auto fcomp = [&](const FSet& f, int ch) {
#pragma unroll
                    for (int kk = 0; kk < GA_SK; ++kk) {
                        const int j = 16 * ch + 4 * kk + (ln >> 4);
                        d2 xh = make_double2(0.0, 0.0);
                        double xv = 0.0;
                        if (j < N) {
                            xh = XH[(size_t)j * GA_RB + (ln & 15)];
                            xv = XV[(size_t)j * GA_RB + (ln & 15)];
                        }
#pragma unroll
                        for (int c = 0; c < GA_RT; ++c) {
                            const d2 v = f.dd[c][kk];
                            cmma(cr[c], ci4[c], v, xh);
                            re[c] = mfma64(v.x * v.x + v.y * v.y, xv, re[c]);
                        }
                    }
                };
                FSet fa, fb;
                fload(fa, wf);
                for (int ch = wf; ch < nch; ch += 2 * GA_WAVES) {
                    fload(fb, ch + GA_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                    fcomp(fa, ch);
                    __builtin_amdgcn_sched_barrier(0);
                    fload(fa, ch + 2 * GA_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                    if (ch + GA_WAVES < nch) fcomp(fb, ch + GA_WAVES);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // ln l, register q: row 16 c + (l >> 4) + 4 q of the 32, realisation l & 15
#pragma unroll
                for (int c = 0; c < GA_RT; ++c)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        double* const o = part + ((size_t)(wf * GA_TR + 16 * c + (ln >> 4) + 4 * q) * GA_RB + (ln & 15)) * 3;
                        o[0] = cr[c][q];
                        o[1] = ci4[c][q];
                        o[2] = re[c][q];
                    }
                __syncthreads();
                {
                    double sx = 0.0, sy = 0.0, sr = 0.0;
#pragma unroll
                    for (int v = 0; v < GA_WAVES; ++v) {
                        const double* const o = part + ((size_t)(v * GA_TR + lt) * GA_RB + lb) * 3;
                        sx += o[0];
                        sy += o[1];
                        sr += o[2];
                    }
                    const int e = GA_TR * rg + lt;
                    if (act && e < d) {
                        AX[e * GA_RB + lb] = make_double2(sx, sy);
                        A2[e * GA_RB + lb] = sr;
                    }
                }
                __syncthreads();
            }

            // ---------------- m-space step
            asm volatile("" : "+v"(ln));
            lb = ln & 15, lt = 4 * w + (ln >> 4);
            double val;
            {
                GA_VECS(wsb, nN, nM)
                double v[1] = {0.0};
                if (act)
                    for (int e = lt; e < d; e += GA_TR) {
                        const int i = e * GA_RB + lb;
                        v[0] += -(cabs2(csub(YM[i], AX[i])) + A2[i]) / wpos;   // CAwgnEstimOut.logLike
                    }
                ga_red(v, red, t);
                val = v[0] + valIn;
            }
            const bool pass = act && (it == 1 || step <= 0.0 || val >= valOpt);
            if (act) {
                if (pass) {
                    valOpt = val;
                    step = fmin(1.1 * fmax(step, 0.0), 1.0);
                } else {
                    step = fmin(fmax(0.0, 0.5 * step), 1.0);
                    if (step < 1e-10) stopnow = true;
                }
            }
            for (int e = lt; e < DP; e += GA_TR) {
                GA_VECS(wsb, nN, nM)
                const int i = e * GA_RB + lb;
                d2 sh = make_double2(0.0, 0.0);
                double sv = 0.0;
                if (act && e < d) {
                    d2 sho, shn;
                    double svo, svn;
                    if (pass) {
                        sho = SH[i];
                        svo = SV[i];
                        const d2 ax = AX[i], y = YM[i];
                        const double a2 = A2[i];
                        const d2 ph_ = csub(ax, cscale(sho, a2));            // phat = Axhat - A2xvar shat
                        const double gain = a2 / (a2 + psi);                 // CAwgnEstimOut.estim
                        const d2 zh = cadd(cscale(csub(y, ph_), gain), ph_);
                        const double zv = psi * gain;
                        shn = cscale(csub(zh, ph_), 1.0 / a2);
                        svn = (1.0 / a2) * (1.0 - zv / a2);
                        if (it == 1 && cold) svo = svn;                      // svar0 missing: "equivalent to step = 1"
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
                    if (fabs(sv) < GA_EPS) sv = GA_EPS;
                    SH[i] = sh;
                    SV[i] = sv;
                }
                shL[lb * ST + e] = sh;
                svL[lb * ST + e] = sv;
            }
            __syncthreads();

            // ---------------- backward sweep: D^H shat, |D|^2^T svar; the input estimator in the epilogue
            asm volatile("" : "+v"(ln));
            int wb = w;
            asm volatile("" : "+s"(wb));
            lb = ln & 15, lt = 4 * wb + (ln >> 4);
            const int frw = (ln & 15) * ST + (ln >> 4);
            double ev[3] = {0.0, 0.0, 0.0};   // valIn, sum |xhatPrev - xhat|^2, sum |xhat|^2
            const double var0 = fmax(GA_EPS, phi), log1m = log(1.0 - lam), logl = log(lam);
            const double lp1 = fmax(1e-8, lam), lp0 = fmax(1e-8, 1.0 - lam);
            const bool first_cold = it == 1 && cold;
            for (int tp = wb; tp < npair; tp += GA_WAVES) {
                GA_VECS(wsb, nN, nM)
                const int j0 = tp * (16 * GA_TW);
                d2 fa[GA_TW][GA_SK], fb[GA_TW][GA_SK];
                d4v cr[GA_TW], ci4[GA_TW], re[GA_TW];
#pragma unroll
                for (int c = 0; c < GA_TW; ++c) cr[c] = ci4[c] = re[c] = d4v{0.0, 0.0, 0.0, 0.0};
                auto gload = [&](d2(&f)[GA_TW][GA_SK], int s) {
#pragma unroll
                    for (int kk = 0; kk < GA_SK; ++kk) {
                        const int e = 4 * (GA_SK * s + kk) + (ln >> 4);
#pragma unroll
                        for (int c = 0; c < GA_TW; ++c) {
                            const int j = j0 + 16 * c + (ln & 15);
                            f[c][kk] = make_double2(0.0, 0.0);
                            if (e < d && j < N) f[c][kk] = D[(size_t)e * N + j];
                        }
                    }
                };
                auto comp = [&](const d2(&f)[GA_TW][GA_SK], int s) {
#pragma unroll
                    for (int kk = 0; kk < GA_SK; ++kk) {
                        const d2 r = shL[frw + 4 * (GA_SK * s + kk)];
                        const double rv = svL[frw + 4 * (GA_SK * s + kk)];
#pragma unroll
                        for (int c = 0; c < GA_TW; ++c) {
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
                // ln l, register q: atom j0 + 16 c + (l >> 4) + 4 q, realisation l & 15
                // (one copy of the estimator's code, the accumulators picked by selects: the unrolled form spills)
                if (act) {
#pragma unroll 1
                    for (int cq = 0; cq < 4 * GA_TW; ++cq) {
                            const int c = cq >> 2, q = cq & 3;
                            const int j = j0 + 16 * c + (ln >> 4) + 4 * q;
                            const double acr = ga_pick(cr, cq), aci = ga_pick(ci4, cq), are = ga_pick(re, cq);
                            if (j < N) {
                                const size_t i = (size_t)j * GA_RB + lb;
                                d2 xo, xdo;
                                if (pass) {
                                    const d2 prev = XO[i];
                                    xo = XH[i];
                                    ev[1] += cabs2(csub(prev, xo));
                                    ev[2] += cabs2(xo);
                                    xdo = first_cold ? xo : XD[i];   // xhatPrev0 missing: "equivalent to step = 1"
                                    XO[i] = xo;
                                    XDO[i] = xdo;
                                    XVF[i] = XV[i];
                                    RHF[i] = RH[i];
                                    RVF[i] = RV[i];
                                } else {
                                    xo = XO[i];
                                    xdo = XDO[i];
                                }
                                const d2 xd = cadd(cscale(xdo, 1.0 - step), cscale(xo, step));
                                const double rvar = 1.0 / are;
                                const d2 rhat = cadd(xd, cscale(make_double2(acr, aci), rvar));
                                // SparseScaEstim.estim around CAwgnEstimIn (mean0 = 0, var0, p1 = lambda)
                                const double r2 = cabs2(rhat);
                                const double ll1 = -(log(M_PI) + log(var0 + rvar) + r2 / (var0 + rvar));
                                const double rv = rvar < GA_EPS ? GA_EPS : rvar;
                                const double ll0 = -(log(M_PI) + log(rv) + r2 / rv);
                                const double ex = fmax(fmin(ll0 - ll1 + log1m - logl, 500.0), -500.0);
                                const double py1 = 1.0 / (1.0 + exp(ex)), py0 = 1.0 - py1;
                                const double gain = var0 / (var0 + rv);
                                const d2 xh1 = cscale(rhat, gain);
                                const double xv1 = gain * rv, xr = rv / (var0 + rv);
                                const double v1 = log(xr) + (1.0 - xr) - cabs2(xh1) / var0;
                                const d2 xh = cscale(xh1, py1);
                                // (|xh1|^2 - |xh|^2 with both squares in the same form: fused differently, the two leave one
                                // ulp of |xh1|^2 behind where py1 = 1 and the difference is exactly 0, 1e-13 of xvar on an
                                // active atom, and the variance loop of an undamped call multiplies that tenfold per step)
                                const double q1 = ga_abs2_rn(xh1), q = ga_abs2_rn(xh);
                                const double xv = py1 * (q1 - q) + py1 * xv1 + py0 * (0.0 - q);
                                ev[0] += py1 * v1 + py1 * log(lp1 / fmax(py1, 1e-8)) + py0 * log(lp0 / fmax(py0, 1e-8));
                                XD[i] = xd;
                                RH[i] = rhat;
                                RV[i] = rvar;
                                XH[i] = xh;
                                XV[i] = xv;
                            }
                        }
                }
            }
            ga_red(ev, red, t);   // (its barriers also order the epilogue's stores before the next sweep's loads)
            if (act) {
                valIn = ev[0];
                if (pass) {
                    mask |= 1 << (it - 1);
                    ++npass;
                    if (it > 1 && !stopnow && ev[1] / ev[2] < tol2) stopnow = true;
                }
                gstop = stopnow;
            }
        }

        // ================================================= after the call
        int pl = t;
        asm volatile("" : "+v"(pl));
        const int pb = pl & 15, pt = pl >> 4;   // = bc, tr (opaque, as above)
        const long long pbb = (long long)blockIdx.x * GA_RB + pb;
        GA_VECS(wsb, nN, nM)
        if (incall) {
            if (pt == 0 && a.trace) {
                a.trace[((size_t)pbb * (a.max_em + 1) + ci) * 2] = it;
                a.trace[((size_t)pbb * (a.max_em + 1) + ci) * 2 + 1] = mask;
            }
            ++ci;
            cold = false;
        }
        if (ph == 1) {   // the final call: done
            ph = 2;
            ok_out = true;
        }
        // EM update (the realisations with ph == 0)
        const bool em = ph == 0;
        double nv[4] = {0.0, 0.0, 0.0, 0.0}, mv[3] = {0.0, 0.0, 0.0};   // CBG sums, change; NaN count, shat, svar
        if (em && npass >= 2) {
            for (int j = pt; j < N; j += GA_TR) {
                const size_t i = (size_t)j * GA_RB + pb;
                const d2 rh = RHF[i], xo = XO[i];
                const double rv = RVF[i], r2 = cabs2(rh);
                if (isnan(rh.x) || isnan(rh.y)) mv[0] += 1.0;
                const double pvs = phi + rv + GA_EPS;
                const d2 gam = cscale(cscale(rh, phi), 1.0 / pvs);
                const double nu = rv * phi / pvs;
                double An = (1.0 - lam) / lam * phi / nu * exp(r2 / pvs - r2 / rv);
                An = 1.0 / (1.0 + An);
                if (isnan(An)) An = 0.999;
                nv[0] += An * (nu + cabs2(gam));
                nv[1] += An;
                nv[2] += t_em > 1 ? cabs2(csub(xo, XP[i])) : 0.0;
                nv[3] += cabs2(xo);
            }
            for (int e = pt; e < d; e += GA_TR) {
                mv[1] += cabs2(SHO[e * GA_RB + pb]);
                mv[2] += SVO[e * GA_RB + pb];
            }
        }
        ga_red(nv, red, t);
        ga_red(mv, red, t);
        if (em) {
            if (npass < 2 || mv[0] != 0.0) {   // EMGMAMP.m:320: rhat has NaN
                stat |= ACE_ST_GAMP_NANBREAK;
                if (!have_ratio) {
                    stat |= ACE_ST_GAMP_FAILED;   // the post-loop update reads a Shat that was never assigned
                    ph = 2;
                } else {
                    // EMGMAMP.m:320 breaks before optGAMP.warmStart(estFin) (:400): the final call starts from the warm
                    // start taken after the PREVIOUS call, i.e. from this call's entry state, not from what this call
                    // left.  This call's only pass was its forced first one, so the Opt copies and xvarFinal ARE the
                    // entry values of xhat, xvar, xhatDamp, shat, svar; step, valIn and the last passed utility were
                    // kept at the entry.  (A NaN in rhatFinal after two passes cannot arise: a pass after the first
                    // needs a utility that is not NaN, hence an xhat and an rhat without NaN.)
                    for (int j = pt; j < N; j += GA_TR) {
                        const size_t i = (size_t)j * GA_RB + pb;
                        XH[i] = XO[i];
                        XV[i] = XVF[i];
                        XD[i] = XDO[i];
                    }
                    for (int e = pt; e < d; e += GA_TR) {
                        SH[e * GA_RB + pb] = SHO[e * GA_RB + pb];
                        SV[e * GA_RB + pb] = SVO[e * GA_RB + pb];
                    }
                    step = ent[0][pb];
                    valIn = ent[1][pb];
                    valOpt = ent[2][pb];
                    psi *= ratio;
                    ph = 1;
                }
            } else {
                phi = nv[0] / nv[1];
                if (a.learn) lam = nv[1] / N;
                phi = fmax(phi, 1e-5);
                ratio = mv[1] / mv[2];
                have_ratio = true;
                psi *= ratio;
                const double emtol = fmin(psi / sqrt(ny2) / 10.0, 1e-4);
                const double change = t_em > 1 ? nv[2] / nv[3] : INFINITY;
                bool stop = emstop;
                if (change < emtol) stop = true;
                else if (stop) stat |= ACE_ST_GAMP_MAXEM;
                if (stop) {
                    psi *= ratio;   // the post-loop update
                    ph = 1;
                } else {
                    for (int j = pt; j < N; j += GA_TR) XP[(size_t)j * GA_RB + pb] = XO[(size_t)j * GA_RB + pb];
                }
            }
            if (ph != 2 && !(psi >= 0.0)) {   // CAwgnEstimOut's assert
                stat |= ACE_ST_GAMP_FAILED;
                ph = 2;
            }
        }
    }

    // ---------------- outputs
    if (!live) return;
    int ol = t;
    asm volatile("" : "+v"(ol));
    const int ob = ol & 15, ot = ol >> 4;
    const long long obb = (long long)blockIdx.x * GA_RB + ob;
    GA_VECS(wsb, nN, nM)
    for (int j = ot; j < N; j += GA_TR) {
        const size_t i = (size_t)j * GA_RB + ob;
        a.xhat[(size_t)obb * N + j] = ok_out ? XO[i] : make_double2(0.0, 0.0);
        if (a.xvar) a.xvar[(size_t)obb * N + j] = ok_out ? XVF[i] : 0.0;
    }
    if (ot == 0) {
        a.params[obb * 3] = lam;
        a.params[obb * 3 + 1] = phi;
        a.params[obb * 3 + 2] = psi;
        a.em_iters[obb] = t_em;
        if (a.status) a.status[obb] = stat;
        if (a.trace)
            for (int c = ci; c <= a.max_em; ++c) a.trace[((size_t)obb * (a.max_em + 1) + c) * 2] = a.trace[((size_t)obb * (a.max_em + 1) + c) * 2 + 1] = 0;
    }
}

int ga_check_args(const ace_gamp_cfg* cfg, int batch, int d, int N, const double* D, const double* Y, const double* xhat,
                  const double* params, const int32_t* em_iters) {
    if (!cfg) return fail(ACE_ERR_ARG, "gamp: NULL cfg");
    if (batch < 1) return fail(ACE_ERR_ARG, "gamp: batch %d < 1", batch);
    if (d < 1 || d > GA_DMAX) return fail(d < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "gamp: d %d outside 1..%d", d, GA_DMAX);
    if (N < 1 || N > GA_NMAX) return fail(N < 1 ? ACE_ERR_ARG : ACE_ERR_UNSUPPORTED, "gamp: N %d outside 1..%d", N, GA_NMAX);
    if (!std::isfinite(cfg->snr_db)) return fail(ACE_ERR_ARG, "gamp: snr_db is not finite");
    if (!(cfg->lambda0 > 0.0 && cfg->lambda0 <= 1.0)) return fail(ACE_ERR_ARG, "gamp: lambda0 %g outside (0, 1]", cfg->lambda0);
    if (cfg->max_em_iter < 0) return fail(ACE_ERR_ARG, "gamp: max_em_iter %d < 0", cfg->max_em_iter);
    if (cfg->gamp_nit < 1 || cfg->gamp_nit > GA_NITMAX)
        return fail(ACE_ERR_ARG, "gamp: gamp_nit %d outside 1..%d", cfg->gamp_nit, GA_NITMAX);
    if (!(cfg->step0 > 0.0 && cfg->step0 <= 1.0)) return fail(ACE_ERR_ARG, "gamp: step0 %g outside (0, 1]", cfg->step0);
    if (!(cfg->gamp_tol >= 0.0)) return fail(ACE_ERR_ARG, "gamp: gamp_tol %g is not >= 0", cfg->gamp_tol);
    if (!D || !Y || !xhat || !params || !em_iters)
        return fail(ACE_ERR_ARG, "gamp: NULL %s", !D ? "D" : !Y ? "Y" : !xhat ? "xhat" : !params ? "params" : "em_iters");
    return ACE_OK;
}

size_t ga_ws_bytes(int batch, int d, int N) {
    const size_t ng = ((size_t)batch + GA_RB - 1) / GA_RB;
    return ((ng * ga_group_doubles(d, N) * sizeof(double) + 255) & ~(size_t)255) + 256;   // (the base is rounded up to 256 B)
}

}  // namespace

size_t gamp_request_bytes(int d) { return ga_lds_bytes(d < 1 ? 1 : d > GA_DMAX ? GA_DMAX : d); }

}  // namespace ace

using namespace ace;

extern "C" void ace_gamp_cfg_default(ace_gamp_cfg* cfg) {
    if (!cfg) return;
    cfg->snr_db = 0.0;
    cfg->lambda0 = 0.0;   // s / n: the caller's
    cfg->learn_lambda = 0;
    cfg->max_em_iter = 200;
    cfg->gamp_nit = 25;
    cfg->reserved = 0;
    cfg->step0 = 0.1;
    cfg->gamp_tol = 1e-5;
}

extern "C" size_t ace_gamp_workspace_size(int batch, int d, int N) {
    if (batch < 1 || d < 1 || d > GA_DMAX || N < 1 || N > GA_NMAX) return 0;
    return ga_ws_bytes(batch, d, N);
}

extern "C" int ace_gamp_solve_batch(const ace_gamp_cfg* cfg, int batch, int d, int N, const double* D, const double* Y,
                                    double* xhat, double* xvar, double* params, int32_t* em_iters, int32_t* trace,
                                    uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(ga_check_args(cfg, batch, d, N, D, Y, xhat, params, em_iters));
    const size_t need = ga_ws_bytes(batch, d, N);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "gamp: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    // 96 KiB of dynamic LDS and more, past the 64 KiB default: the kernel's derived budget decides (no fallback)
    const void* const kern = reinterpret_cast<const void*>(&gamp_kernel);
    const size_t lds = ga_lds_bytes(d);
    if (!lds_ok(kern, lds))
        return fail(ACE_ERR_UNSUPPORTED, "gamp: gamp_kernel needs %zu B of dynamic LDS, budget %zu B", lds, lds_dyn_budget(kern));
    GampArgs a;
    a.batch = batch;
    a.d = d;
    a.N = N;
    a.max_em = cfg->max_em_iter;
    a.nit = cfg->gamp_nit;
    a.learn = cfg->learn_lambda != 0;
    a.snr_lin = 1.0 + std::pow(10.0, std::fmin(100.0, cfg->snr_db) / 10.0);
    a.lam0 = cfg->lambda0;
    a.step0 = cfg->step0;
    a.tol = cfg->gamp_tol;
    a.D = (const d2*)D;
    a.Y = (const d2*)Y;
    a.xhat = (d2*)xhat;
    a.xvar = xvar;
    a.params = params;
    a.em_iters = em_iters;
    a.trace = trace;
    a.status = status;
    a.ws = (double*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int nblk = (batch + GA_RB - 1) / GA_RB;
    hipLaunchKernelGGL(gamp_kernel, dim3(nblk), dim3(GA_NT), lds, (hipStream_t)stream, a);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}

extern "C" int ace_gamp_solve_host(const ace_gamp_cfg* cfg, int batch, int d, int N, const double* D, const double* Y,
                                   double* xhat, double* xvar, double* params, int32_t* em_iters, int32_t* trace,
                                   uint32_t* status) {
    g_err.clear();
    ACE_TRY(ga_check_args(cfg, batch, d, N, D, Y, xhat, params, em_iters));
    const size_t B = batch, wsb = ga_ws_bytes(batch, d, N), ntr = 2 * B * ((size_t)cfg->max_em_iter + 1);
    DevScope dev;
    double *dD, *dY, *dxhat, *dxvar = nullptr, *dpar;
    int32_t *dem, *dtr = nullptr;
    uint32_t* dst = nullptr;
    char* dws;
    ACE_TRY(dev.put(&dD, D, 2 * (size_t)d * N));
    ACE_TRY(dev.put(&dY, Y, 2 * B * d));
    ACE_TRY(dev.alloc(&dxhat, 2 * B * N));
    if (xvar) ACE_TRY(dev.alloc(&dxvar, B * N));
    ACE_TRY(dev.alloc(&dpar, 3 * B));
    ACE_TRY(dev.alloc(&dem, B));
    if (trace) ACE_TRY(dev.alloc(&dtr, ntr));
    if (status) ACE_TRY(dev.alloc(&dst, B));
    ACE_TRY(dev.alloc(&dws, wsb));
    ACE_TRY(ace_gamp_solve_batch(cfg, batch, d, N, dD, dY, dxhat, dxvar, dpar, dem, dtr, dst, dws, wsb, nullptr));
    ACE_HIP(hipDeviceSynchronize());
    ACE_TRY(dev.get(xhat, dxhat, 2 * B * N));
    ACE_TRY(dev.get(xvar, dxvar, B * N));
    ACE_TRY(dev.get(params, dpar, 3 * B));
    ACE_TRY(dev.get(em_iters, dem, B));
    ACE_TRY(dev.get(trace, dtr, ntr));
    return dev.get(status, dst, B);
}
