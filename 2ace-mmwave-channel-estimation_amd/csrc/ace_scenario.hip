// The reference's Monte-Carlo scenarios on the device: Generate_Channel.m:64-142 and Generate_Measurement.m:67-118
// restated in full, for a batch of realisations, with every measurement kind at its own scale.
//
//   channel  AoD, AoA of the L dominant paths ~ U(-Searching_Area/2, Searching_Area/2) degrees (:78-79; fix_angle:
//            0 and 15, :73-75); on_grid snaps sin(angle) to linspace(-1,1,NQ+1)(1:end-1), the nearest point and the
//            first on a tie (MATLAB's min, :89-94), and the angle becomes asind of it; gains CN(0,1) normalised to
//            unit norm (:98-99).  With L == 1, Rician_K further paths: gains CN normalised (:107-108), angles
//            ~ U(-pi/2, pi/2) radians (:110-111).  H = sqrt(Nt Nr) ARx diag(h) ATx' per group (:120, :129), mixed as
//            sqrt(K/(K+1)) H_dominant + sqrt(1/(K+1)) H_nlos with K = 10^(7/10) when Rician_K != 0 (:132-138).
//            Entry H[r][t] = sum_p g_p exp(j kappa (sin(AoD_p) t - sin(AoA_p) r)), vecH[r + Nr t] (ace_synth.hip's order).
//   measure  y = FW vecH + noiseVec (:100); noiseVec = diag(W' * noiseMatrix) repeated once per Tx beam (:92-97),
//            noiseMatrix Nr x Mr iid CN(0, noise_power): noise(it Mr + q) = sum_r conj(W[q][r]) N[r][q] (noise model
//            1), or iid CN(0, noise_power) per probe (noise model 0, what ace_synth_channels draws); Add_Noise_Flag = 0:
//            y = FW vecH (:105-112).  y_noisy = y .* CN(0,1) (:102-103).  B_raw = |y|, scale = ||B_raw||.
//   scaled   B = B_raw / scale, X0 = (vecH + x0_noise ||vecH|| / sqrt(n) CN(0,1)) / scale, Hn = vecH / scale (what
//            InferADMM's inputs get, inferLowRankV4_multi.m:32-38, and ace_synth_channels returns).
//
// Random streams: ace_synth.hip's counter generator.  Kinds 2 (angles: AoD at counters 0 .. L-1, AoA at L .. 2L-1),
// 3 (gains), 4 (iid noise, counter = probe) and 5 (X0) keep their meaning, so the default cfg draws
// ace_synth_channels' numbers; 10 NLOS angles (AoD at 0 .. Rk-1, AoA at Rk .. 2Rk-1), 11 NLOS gains, 12 phase noise
// (counter = probe), 13 combiner noise matrix (counter = q rx + r).
//
// Kernels, in stream order; no atomics, every sum has a fixed order, nothing spins across work-groups.
//   sc_draws_kernel    one thread per realisation: angles, snapped sines and gains into the workspace record (the
//                      gains with their K-factor weights) and into `paths` (without).
//   sc_channel_kernel  one work-group per realisation: vecH (one sincos per path and entry), ||H||, and for noise
//                      model 1 the Mr combiner-noise values.
//   sc_prod_kernel     shared A: Y[count][m] = vecH A^T is one complex product over the whole call on
//                      v_mfma_f64_16x16x4_f64 in the 4M form (cmma of ace_mfma.hpp).  A work-group (4 waves) owns a tile
//                      of 16 realisations x 16 probes; its waves split k in chunks of 16 (wave w: chunks w, w + 4, ...),
//                      each lane loading 4 consecutive entries (64 B) of its realisation's vecH and of its probe's row
//                      per chunk straight from global memory, as ace_aopt.hip's candidate sweep does; the four partial
//                      tiles are added through LDS in wave order.  The epilogue (wave 0) adds the noise, writes y,
//                      y_noisy and B_raw and leaves one partial sum of |y|^2 per realisation and tile (a 16-lane
//                      butterfly).  Entries k >= n, probes >= m and realisations >= count are masked at the loads.
//   sc_priv_kernel     private codebooks: the per-realisation product, one work-group each, one wave per probe (lane
//                      partial sums over k = lane + 64 j, then a butterfly), as channel_kernel of ace_synth.hip has
//                      it; one partial sum of |y|^2 per realisation.
//   sc_finish_kernel   one work-group per realisation: scale from the partials in tile order, then B, X0, Hn.
//
// Batch invariance: a realisation's outputs are a function of (cfg, seed, its index, A, W) alone.  Its row of an
// MFMA tile does not depend on the other rows, the chunk walk depends on n only, the tile walk on m only, and every
// draw is addressed by the realisation's index.
//
// Resources as compiled: DESIGN.md §4k.
#include "ace_common.hpp"
#include "ace_host.hpp"
#include "ace_mfma.hpp"

namespace ace {
namespace {

constexpr int SC_ANT = 32;        // largest tx, rx
constexpr int SC_MMAX = 4096;     // largest m
constexpr int SC_LMAX = 8;        // largest L
constexpr int SC_RKMAX = 16;      // largest rician_k
constexpr int SC_NQMAX = 65536;   // largest NQt, NQr
constexpr int SC_PMAX = SC_RKMAX + 1 > SC_LMAX ? SC_RKMAX + 1 : SC_LMAX;   // paths of one channel
constexpr int SC_REC = 4 * SC_PMAX;   // doubles of a realisation's record: sin AoD [P], sin AoA [P], weighted gains [2P]
constexpr int SC_WAVES = 4;
constexpr int SC_NT = 64 * SC_WAVES;

enum { SC_ANGLES = 2, SC_GAINS = 3, SC_NOISE = 4, SC_X0 = 5, SC_NLOS_ANGLES = 10, SC_NLOS_GAINS = 11, SC_PHASE = 12,
       SC_COMBINER = 13 };

// ace_synth.hip's generator (splitmix64 of seed / stream / counter; Box-Muller pairs from counters 2c, 2c + 1)
__device__ __forceinline__ uint64_t sc_sm64(uint64_t seed, uint64_t stream, uint64_t ctr) {
    uint64_t z = (seed ^ (stream * 0xD1B54A32D192ED03ULL)) + (ctr + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double sc_u01(uint64_t seed, uint64_t stream, uint64_t ctr) {
    return (double)(sc_sm64(seed, stream, ctr) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ d2 sc_nrm2(uint64_t seed, uint64_t stream, uint64_t c) {
    const double u1 = sc_u01(seed, stream, 2 * c), u2 = sc_u01(seed, stream, 2 * c + 1);
    const double r = sqrt(-2.0 * log(1.0 - u1));
    double s, co;
    sincos(2.0 * M_PI * u2, &s, &co);
    return make_double2(r * co, r * s);
}
__device__ __forceinline__ uint64_t sc_stream(int kind, long long real) {
    return (uint64_t)kind + 16ULL * (uint64_t)(real + 1);
}

struct ScP {   // one call's parameters, by value to every kernel
    uint64_t seed;
    long long first;
    int count, m, tx, rx, n, Mr, a_shared;
    int L, Rk, P;   // dominant paths, NLOS paths in effect, L + Rk
    int on_grid, fix_angle, NQt, NQr, add_noise, noise_model;
    double search_deg, wd, wn;   // K-factor weights of the two groups (1, 0 without NLOS paths)
    double ns;                   // sqrt(sigma2 / 2)
    double x0_noise, kap;        // kappa = 2 pi d / lambda
};

struct ScBufs {
    double* rec;    // [count][SC_REC]
    double* nH;     // [count] ||vecH||
    d2* H;          // [count][n] (when the caller takes no vecH)
    double* Braw;   // [count][m] (when the caller takes no B_raw)
    double* part;   // [count][ntile] partial sums of |y|^2
    d2* nv;         // [count][Mr] combiner noise (noise model 1)
};

constexpr int sc_ntile(int m) { return (m + 15) / 16; }

void sc_carve(Carver& cv, int count, int m, int n, int Mr, ScBufs* b) {
    const size_t C = count;
    b->rec = cv.take<double>(C * SC_REC * sizeof(double));
    b->nH = cv.take<double>(C * sizeof(double));
    b->H = cv.take<d2>(C * n * sizeof(d2));
    b->Braw = cv.take<double>(C * m * sizeof(double));
    b->part = cv.take<double>(C * sc_ntile(m) * sizeof(double));
    b->nv = cv.take<d2>(C * (Mr > 0 ? Mr : 0) * sizeof(d2));
}

// the grid point p (2 / NQ) - 1 (p = 0 .. NQ - 1; linspace's own arithmetic, each step rounded, so the points are
// angular.grid_cut's bit for bit) nearest s, the first on a tie: the minimum lies within one point of
// floor((s + 1) NQ / 2), so four candidates in ascending order under a strict comparison give MATLAB's min
__device__ __forceinline__ double sc_snap(double s, int NQ) {
    const int p0 = (int)floor((s + 1.0) * 0.5 * NQ);
    const int lo = max(min(p0 - 1, NQ - 1), 0), hi = max(min(p0 + 2, NQ - 1), 0);
    double best = 0.0, bg = 0.0;
    for (int p = lo; p <= hi; ++p) {
        const double g = __dadd_rn(__dmul_rn((double)p, 2.0 / NQ), -1.0);
        const double v = fabs(g - s);
        if (p == lo || v < best) {
            best = v;
            bg = g;
        }
    }
    return bg;
}

// a group's CN gains normalised to unit norm: (re, im) of gain l times wgt into rw[2 l], unweighted into o[2 l]
// (o may be null).  The draws are formed twice, so no per-thread array is indexed at run time (no scratch).
__device__ __forceinline__ void sc_gains(uint64_t seed, uint64_t stream, int cnt, double wgt, bool weighted,
                                         double* __restrict__ rw, double* __restrict__ o) {
    double nn = 0.0;
    for (int l = 0; l < cnt; ++l) {
        const d2 z = sc_nrm2(seed, stream, l);
        const double gx = z.x * M_SQRT1_2, gy = z.y * M_SQRT1_2;
        nn += gx * gx + gy * gy;
    }
    const double inn = 1.0 / sqrt(nn);
    for (int l = 0; l < cnt; ++l) {
        const d2 z = sc_nrm2(seed, stream, l);
        const double gx = z.x * M_SQRT1_2 * inn, gy = z.y * M_SQRT1_2 * inn;
        rw[2 * l] = weighted ? wgt * gx : gx;
        rw[2 * l + 1] = weighted ? wgt * gy : gy;
        if (o) {
            o[2 * l] = gx;
            o[2 * l + 1] = gy;
        }
    }
}

__global__ __launch_bounds__(256) void sc_draws_kernel(ScP p, double* __restrict__ rec, double* __restrict__ paths) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.count) return;
    const long long real = p.first + c;
    const int L = p.L, Rk = p.Rk, P = p.P;
    double* r = rec + (size_t)c * SC_REC;
    double* o = paths ? paths + (size_t)c * 4 * P : nullptr;
    for (int l = 0; l < L; ++l) {
        double aod = (sc_u01(p.seed, sc_stream(SC_ANGLES, real), l) - 0.5) * p.search_deg;
        double aoa = (sc_u01(p.seed, sc_stream(SC_ANGLES, real), L + l) - 0.5) * p.search_deg;
        if (p.fix_angle) {
            aod = 0.0;
            aoa = 15.0;
        }
        if (p.on_grid) {
            aod = asin(sc_snap(sin(aod * M_PI / 180.0), p.NQt)) * (180.0 / M_PI);
            aoa = asin(sc_snap(sin(aoa * M_PI / 180.0), p.NQr)) * (180.0 / M_PI);
        }
        r[l] = sin(aod * M_PI / 180.0);
        r[P + l] = sin(aoa * M_PI / 180.0);
        if (o) {
            o[l] = aod;
            o[L + l] = aoa;
        }
    }
    sc_gains(p.seed, sc_stream(SC_GAINS, real), L, p.wd, Rk != 0, r + 2 * P, o ? o + 2 * L : nullptr);
    if (Rk == 0) return;
    for (int k = 0; k < Rk; ++k) {
        const double aod = (sc_u01(p.seed, sc_stream(SC_NLOS_ANGLES, real), k) - 0.5) * M_PI;
        const double aoa = (sc_u01(p.seed, sc_stream(SC_NLOS_ANGLES, real), Rk + k) - 0.5) * M_PI;
        r[L + k] = sin(aod);
        r[P + L + k] = sin(aoa);
        if (o) {
            o[4 * L + k] = aod;
            o[4 * L + Rk + k] = aoa;
        }
    }
    sc_gains(p.seed, sc_stream(SC_NLOS_GAINS, real), Rk, p.wn, true, r + 2 * P + 2 * L, o ? o + 4 * L + 2 * Rk : nullptr);
}

// one work-group per realisation: vecH, ||vecH|| and the combiner noise
__global__ __launch_bounds__(256) void sc_channel_kernel(ScP p, const double* __restrict__ rec, const d2* __restrict__ W,
                                                         d2* __restrict__ H, double* __restrict__ nH, d2* __restrict__ nv) {
    __shared__ double rs[SC_REC];
    __shared__ double red[16];
    const int c = blockIdx.x, P = p.P, n = p.n;
    const long long real = p.first + c;
    for (int e = threadIdx.x; e < 4 * P; e += 256) rs[e] = rec[(size_t)c * SC_REC + e];
    __syncthreads();
    double v[1] = {0.0};
    for (int k = threadIdx.x; k < n; k += 256) {
        const int r = k % p.rx, t = k / p.rx;
        d2 s = make_double2(0.0, 0.0);
        for (int l = 0; l < P; ++l) {
            const double ph = p.kap * (rs[l] * t - rs[P + l] * r);
            double sn, cs;
            sincos(ph, &sn, &cs);
            s = cadd(s, cmul(make_double2(rs[2 * P + 2 * l], rs[2 * P + 2 * l + 1]), make_double2(cs, sn)));
        }
        H[(size_t)c * n + k] = s;
        v[0] += cabs2(s);
    }
    block_sum(v, red);
    if (threadIdx.x == 0) nH[c] = sqrt(v[0]);
    if (p.add_noise && p.noise_model == 1) {
        for (int q = threadIdx.x; q < p.Mr; q += 256) {
            d2 s = make_double2(0.0, 0.0);
            for (int r = 0; r < p.rx; ++r) {
                const d2 z = sc_nrm2(p.seed, sc_stream(SC_COMBINER, real), (uint64_t)q * p.rx + r);
                s = cadd(s, cmulc(W[(size_t)q * p.rx + r], cscale(z, p.ns)));
            }
            nv[(size_t)c * p.Mr + q] = s;
        }
    }
}

// probe i of realisation c: the noise, then y, y_noisy and B_raw; returns |y|^2
__device__ __forceinline__ double sc_emit(const ScP& p, int c, int i, d2 ah, const d2* __restrict__ nv, d2* __restrict__ y,
                                          d2* __restrict__ yn, double* __restrict__ Braw) {
    const long long real = p.first + c;
    d2 v = ah;
    if (p.add_noise) {
        const d2 w = p.noise_model == 1 ? nv[(size_t)c * p.Mr + i % p.Mr]
                                        : cscale(sc_nrm2(p.seed, sc_stream(SC_NOISE, real), i), p.ns);
        v = cadd(v, w);
    }
    const size_t o = (size_t)c * p.m + i;
    if (y) y[o] = v;
    if (yn) yn[o] = cmul(v, cscale(sc_nrm2(p.seed, sc_stream(SC_PHASE, real), i), M_SQRT1_2));
    const double a2 = cabs2(v);
    Braw[o] = sqrt(a2);
    return a2;
}

// (cr, ci) += D[row][col] = sum_k A[row][k] B[col][k] over the chunks c0, c0 + cs, ... of 16 k: ace_aopt.hip's
// ao_tile.  ap / bp: the lane's operand rows (row l & 15 of each; nullptr: a zero row).  Lane l carries
// k = 16 c + 4 (l >> 4) + kk in k-step kk of chunk c; result: lane l, register q holds D[(l >> 4) + 4 q][l & 15].
__device__ __forceinline__ void sc_tile(const d2* ap, const d2* bp, int n, int c0, int cs, int lane, d4v& cr, d4v& ci) {
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
        for (int kk = 0; kk < 4; ++kk) cmma(cr, ci, a0[kk], b0[kk]);
        if (more) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                a0[kk] = a1[kk];
                b0[kk] = b1[kk];
            }
        }
    }
}

// Grid (tiles of 16 realisations, tiles of 16 probes)
__global__ __launch_bounds__(SC_NT) void sc_prod_kernel(ScP p, const d2* __restrict__ A, const d2* __restrict__ H,
                                                        const d2* __restrict__ nv, d2* __restrict__ y, d2* __restrict__ yn,
                                                        double* __restrict__ Braw, double* __restrict__ part) {
    __shared__ double ps[SC_WAVES - 1][8][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 16, i0 = blockIdx.y * 16;
    const int rc = c0 + (lane & 15), ri = i0 + (lane & 15);
    const d2* ap = rc < p.count ? H + (size_t)rc * p.n : nullptr;
    const d2* bp = ri < p.m ? A + (size_t)ri * p.n : nullptr;
    d4v cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
    sc_tile(ap, bp, p.n, w, SC_WAVES, lane, cr, ci);
    if (w > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ps[w - 1][q][lane] = cr[q];
            ps[w - 1][4 + q][lane] = ci[q];
        }
    }
    __syncthreads();
    if (w > 0) return;
#pragma unroll
    for (int v = 0; v < SC_WAVES - 1; ++v)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cr[q] += ps[v][q][lane];
            ci[q] += ps[v][4 + q][lane];
        }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = c0 + (lane >> 4) + 4 * q;
        double a2 = 0.0;
        if (c < p.count && ri < p.m) a2 = sc_emit(p, c, ri, make_double2(cr[q], ci[q]), nv, y, yn, Braw);
        a2 = bsum16(a2);   // over the tile's 16 probes, the same association for every realisation
        if ((lane & 15) == 0 && c < p.count) part[(size_t)c * gridDim.y + blockIdx.y] = a2;
    }
}

// private codebooks: one work-group per realisation, one wave per probe
__global__ __launch_bounds__(256) void sc_priv_kernel(ScP p, const d2* __restrict__ A, const d2* __restrict__ H,
                                                      const d2* __restrict__ nv, d2* __restrict__ y, d2* __restrict__ yn,
                                                      double* __restrict__ Braw, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char sc_lds[];
    d2* h = reinterpret_cast<d2*>(sc_lds);                  // [n]
    double* ysq = reinterpret_cast<double*>(h + p.n);       // [m]
    __shared__ double red[16];
    const int c = blockIdx.x, n = p.n, m = p.m;
    for (int k = threadIdx.x; k < n; k += 256) h[k] = H[(size_t)c * n + k];
    __syncthreads();
    const d2* Ac = A + (size_t)c * m * n;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = wv; i < m; i += 4) {
        d2 s = make_double2(0.0, 0.0);
        for (int k = lane; k < n; k += 64) s = cadd(s, cmul(Ac[(size_t)i * n + k], h[k]));
        s.x = wave_sum(s.x);
        s.y = wave_sum(s.y);
        if (lane == 0) ysq[i] = sc_emit(p, c, i, s, nv, y, yn, Braw);
    }
    __syncthreads();
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < m; i += 256) v[0] += ysq[i];
    block_sum(v, red);
    if (threadIdx.x == 0) part[c] = v[0];
}

// one work-group per realisation: scale from the partials in tile order, then the normalised outputs
__global__ __launch_bounds__(256) void sc_finish_kernel(ScP p, int npart, const double* __restrict__ part,
                                                        const d2* __restrict__ H, const double* __restrict__ nH,
                                                        const double* __restrict__ Braw, double* __restrict__ scale,
                                                        double* __restrict__ B, d2* __restrict__ X0, d2* __restrict__ Hn) {
    const int c = blockIdx.x, n = p.n, m = p.m;
    const long long real = p.first + c;
    double s2 = 0.0;
    for (int t = 0; t < npart; ++t) s2 += part[(size_t)c * npart + t];   // (every thread: the same sum)
    const double sc = sqrt(s2), inv = sc > 0.0 ? 1.0 / sc : 0.0;
    if (threadIdx.x == 0 && scale) scale[c] = sc;
    if (B)
        for (int i = threadIdx.x; i < m; i += 256) B[(size_t)c * m + i] = Braw[(size_t)c * m + i] * inv;
    if (!X0 && !Hn) return;
    // X0 = vecH + x0_noise * ||vecH|| / sqrt(n) * CN(0,1)
    const double xs = p.x0_noise * nH[c] / sqrt((double)n) * M_SQRT1_2;
    for (int k = threadIdx.x; k < n; k += 256) {
        const d2 h = H[(size_t)c * n + k];
        if (Hn) Hn[(size_t)c * n + k] = cscale(h, inv);
        if (X0) {
            const d2 z = sc_nrm2(p.seed, sc_stream(SC_X0, real), k);
            X0[(size_t)c * n + k] = cscale(cadd(h, cscale(z, xs)), inv);
        }
    }
}

bool sc_cfg_limits(const ace_scenario_cfg* c) {
    return c && c->L >= 1 && c->L <= SC_LMAX && c->rician_k >= 0 && c->rician_k <= SC_RKMAX && c->NQt >= 0 &&
           c->NQt <= SC_NQMAX && c->NQr >= 0 && c->NQr <= SC_NQMAX;
}
bool sc_limits(int count, int m, int tx, int rx) {
    return count >= 1 && m >= 1 && m <= SC_MMAX && tx >= 1 && tx <= SC_ANT && rx >= 1 && rx <= SC_ANT;
}

int sc_range(const char* name, int v, int lo, int hi) {
    if (v < lo) return fail(ACE_ERR_ARG, "scenario: %s %d below %d", name, v, lo);
    if (v > hi) return fail(ACE_ERR_UNSUPPORTED, "scenario: %s %d outside %d..%d", name, v, lo, hi);
    return ACE_OK;
}

int sc_check_args(const ace_scenario_cfg* cfg, int64_t first, int count, int m, int tx, int rx, const double* A,
                  const double* W, int Mr) {
    if (!cfg) return fail(ACE_ERR_ARG, "scenario: NULL cfg");
    if (count < 1) return fail(ACE_ERR_ARG, "scenario: count %d < 1", count);
    if (first < 0) return fail(ACE_ERR_ARG, "scenario: first %lld < 0", (long long)first);
    ACE_TRY(sc_range("tx", tx, 1, SC_ANT));
    ACE_TRY(sc_range("rx", rx, 1, SC_ANT));
    ACE_TRY(sc_range("m", m, 1, SC_MMAX));
    ACE_TRY(sc_range("L", cfg->L, 1, SC_LMAX));
    ACE_TRY(sc_range("rician_k", cfg->rician_k, 0, SC_RKMAX));
    ACE_TRY(sc_range("NQt", cfg->NQt, 0, SC_NQMAX));
    ACE_TRY(sc_range("NQr", cfg->NQr, 0, SC_NQMAX));
    if (cfg->fix_angle && cfg->L != 1) return fail(ACE_ERR_ARG, "scenario: fix_angle needs L == 1 (got L %d)", cfg->L);
    if (cfg->noise_model != 0 && cfg->noise_model != 1)
        return fail(ACE_ERR_ARG, "scenario: noise_model %d is neither 0 nor 1", cfg->noise_model);
    if (!(cfg->search_deg > 0.0) || !(cfg->search_deg <= 180.0))
        return fail(ACE_ERR_ARG, "scenario: search_deg %g outside (0, 180]", cfg->search_deg);
    if (!std::isfinite(cfg->snr_db)) return fail(ACE_ERR_ARG, "scenario: snr_db %g is not finite", cfg->snr_db);
    if (!std::isfinite(cfg->k_factor_db)) return fail(ACE_ERR_ARG, "scenario: k_factor_db %g is not finite", cfg->k_factor_db);
    if (!(cfg->x0_noise >= 0.0) || !std::isfinite(cfg->x0_noise))
        return fail(ACE_ERR_ARG, "scenario: x0_noise %g is not finite and >= 0", cfg->x0_noise);
    if (!(cfg->ant_d > 0.0) || !std::isfinite(cfg->ant_d))
        return fail(ACE_ERR_ARG, "scenario: ant_d %g is not positive and finite", cfg->ant_d);
    if (!(cfg->lambda > 0.0) || !std::isfinite(cfg->lambda))
        return fail(ACE_ERR_ARG, "scenario: lambda %g is not positive and finite", cfg->lambda);
    if (!A) return fail(ACE_ERR_ARG, "scenario: NULL A");
    if (cfg->noise_model == 1) {
        if (!W) return fail(ACE_ERR_ARG, "scenario: noise_model 1 needs W");
        if (Mr < 1) return fail(ACE_ERR_ARG, "scenario: noise_model 1 needs Mr >= 1 (got %d)", Mr);
        if (m % Mr != 0) return fail(ACE_ERR_ARG, "scenario: noise_model 1 needs m %% Mr == 0 (got m %d, Mr %d)", m, Mr);
    }
    return ACE_OK;
}

size_t sc_ws_bytes(const ace_scenario_cfg* cfg, int count, int m, int n, int Mr) {
    Carver cv{nullptr};
    ScBufs b;
    sc_carve(cv, count, m, n, cfg->noise_model == 1 ? Mr : 0, &b);
    return cv.off + 256;   // (the base is rounded up to 256 B)
}

}  // namespace
}  // namespace ace

using namespace ace;

extern "C" void ace_scenario_cfg_default(ace_scenario_cfg* cfg) {
    if (!cfg) return;
    cfg->L = 3;
    cfg->rician_k = 0;
    cfg->on_grid = 0;
    cfg->fix_angle = 0;
    cfg->NQt = cfg->NQr = 0;
    cfg->add_noise = 1;
    cfg->noise_model = 0;
    cfg->search_deg = 95.0;    // channel_recovery_ADMM_v2_simulation_A2only.m:52
    cfg->k_factor_db = 7.0;    // Generate_Channel.m:132
    cfg->snr_db = 30.0;
    cfg->x0_noise = 0.5;
    cfg->ant_d = 3.055e-3;     // A2only.m:40-41
    cfg->lambda = 3e8 / 60.48e9;
}

extern "C" size_t ace_synth_scenario_workspace_size(const ace_scenario_cfg* cfg, int count, int m, int tx, int rx, int Mr) {
    if (!sc_cfg_limits(cfg) || !sc_limits(count, m, tx, rx)) return 0;
    if (cfg->noise_model != 0 && (cfg->noise_model != 1 || Mr < 1 || m % Mr != 0)) return 0;
    return sc_ws_bytes(cfg, count, m, tx * rx, Mr);
}

extern "C" int ace_synth_scenario(const ace_scenario_cfg* cfg, uint64_t seed, int64_t first, int count, int m, int tx,
                                  int rx, const double* A, int a_shared, const double* W, int Mr, double* vecH, double* y,
                                  double* y_noisy, double* B_raw, double* scale, double* B, double* X0, double* Hn,
                                  double* paths, void* workspace, size_t workspace_bytes, void* stream) {
    g_err.clear();
    ACE_TRY(sc_check_args(cfg, first, count, m, tx, rx, A, W, Mr));
    const int n = tx * rx;
    const int mr = cfg->noise_model == 1 ? Mr : 0;
    const size_t need = sc_ws_bytes(cfg, count, m, n, Mr);
    if (!workspace || workspace_bytes < need)
        return fail(ACE_ERR_WORKSPACE, "scenario: workspace of %zu B, need %zu B", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t s = (hipStream_t)stream;
    Carver cv{(char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255)};
    ScBufs b;
    sc_carve(cv, count, m, n, mr, &b);

    ScP p = {};
    p.seed = seed;
    p.first = first;
    p.count = count;
    p.m = m;
    p.tx = tx;
    p.rx = rx;
    p.n = n;
    p.Mr = mr > 0 ? mr : 1;
    p.a_shared = a_shared;
    p.L = cfg->L;
    p.Rk = cfg->L == 1 ? cfg->rician_k : 0;
    p.P = p.L + p.Rk;
    p.on_grid = cfg->on_grid != 0;
    p.fix_angle = cfg->fix_angle != 0;
    p.NQt = cfg->NQt ? cfg->NQt : 4 * tx;
    p.NQr = cfg->NQr ? cfg->NQr : 4 * rx;
    p.add_noise = cfg->add_noise != 0;
    p.noise_model = cfg->noise_model;
    p.search_deg = cfg->search_deg;
    const double K = pow(10.0, cfg->k_factor_db / 10.0);
    p.wd = p.Rk ? sqrt(K / (K + 1.0)) : 1.0;
    p.wn = p.Rk ? sqrt(1.0 / (K + 1.0)) : 0.0;
    p.ns = sqrt(pow(10.0, -cfg->snr_db / 10.0)) * M_SQRT1_2;
    p.x0_noise = cfg->x0_noise;
    p.kap = 2.0 * M_PI * (cfg->ant_d / cfg->lambda);

    d2* H = vecH ? (d2*)vecH : b.H;
    double* Braw = B_raw ? B_raw : b.Braw;
    const dim3 blk(256);
    hipLaunchKernelGGL(sc_draws_kernel, dim3((count + 255) / 256), blk, 0, s, p, b.rec, paths);
    hipLaunchKernelGGL(sc_channel_kernel, dim3(count), blk, 0, s, p, b.rec, (const d2*)W, H, b.nH, b.nv);
    int npart;
    if (a_shared) {
        npart = sc_ntile(m);
        hipLaunchKernelGGL(sc_prod_kernel, dim3((count + 15) / 16, npart), dim3(SC_NT), 0, s, p, (const d2*)A, H, b.nv,
                           (d2*)y, (d2*)y_noisy, Braw, b.part);
    } else {
        npart = 1;
        const size_t lds = (size_t)n * sizeof(d2) + (size_t)m * sizeof(double);   // <= 16 KiB + 32 KiB
        hipLaunchKernelGGL(sc_priv_kernel, dim3(count), blk, lds, s, p, (const d2*)A, H, b.nv, (d2*)y, (d2*)y_noisy, Braw,
                           b.part);
    }
    hipLaunchKernelGGL(sc_finish_kernel, dim3(count), blk, 0, s, p, npart, b.part, H, b.nH, Braw, scale, B, (d2*)X0,
                       (d2*)Hn);
    ACE_HIP(hipGetLastError());
    return ACE_OK;
}
