/*
 * ace.h -- C-ABI of the MI355X-native 2ACE ADMM channel-recovery hot path.
 *
 * Reference interfaces replaced (reference root: gavinsyw/2ACE-mmWave-Channel-Estimation):
 *
 *  ace_admm_solve_batch   <- [X,Y,converged] = InferADMM(A,B,X0,scale_by_row,use_rank_one,
 *                            tx,rx,lambda,mu0,rho,tol_rel,tol_abs,maxiter,U,D)
 *                            main/src/my_recovery_algorithms/ADMM_v2/inferLowRankV4_multi.m:281
 *                            (A2only Z-prox :423-485) and inferLowRank_Nuclear.m:269
 *                            (nuclear Z-prox :411-439).  One call solves a batch of
 *                            independent realisations; the refinement stage called at
 *                            inferLowRankV4_multi.m:92 / :100 is r = 1, scale_by_row = 1.
 *  ace_admm_solve_host    <- the same, on host arrays (drop-in for MATLAB Engine calls
 *                            that pass matlab.double buffers; main/main.py:427-437).
 *  ace_pipeline_solve_batch <- [X,Y,quality] = inferLowRankV4_multi(A,B,tx,rx)
 *                            main/src/my_recovery_algorithms/ADMM_v2/inferLowRankV4_multi.m:5-109
 *                            (3 restarts), Numerical_Simulation/.../inferLowRankV4.m (1 restart)
 *                            and inferLowRank_Nuclear.m (1 restart, nuclear Z-prox), as called by
 *                            ADMM_v2(meas,FW,TX,RX,version) (ADMM_v2.m:30-32) and
 *                            ADMM_v2_nuclear.m:30-32.  Spectral initialisation (:561-574),
 *                            inferLowRankImpl (:111-271: r = 20 row-scaled stage, rotation by
 *                            eig(X'X), per-column stage), test quality and rank-one retry
 *                            (:68-77), best of restarts (:79-83), refinement (:89-101),
 *                            rollback and rescale (:93-107) -- all on the GPU.
 *  ace_phaselift_solve_batch <- recoveredSig = MyPhaseLift(measurements, measurementMat)
 *                            main/src/my_recovery_algorithms/MyPhaseLift.m:69-107 (TFOCS
 *                            solver_TraceLS + tfocs_AT, prox_trace), batched over realisations.
 *  ace_recover_driver     <- [H_amp,H_angle] = channel_recovery_ADMM_v2_simulation_A2only /
 *                            _A2nuclear / _multiresolution(tx,rx,cb_amp,cb_angle,rss_final,
 *                            seed_id)  main/channel_recovery_ADMM_v2_simulation_A2only.m:9,
 *                            called from main/main.py:427-437 through the MATLAB Engine.
 *  ace_synth_*            <- synthetic trace generation with the semantics of
 *                            main/src/generate_channel/Generate_Channel.m:64-164,
 *                            generate_sensing_matrix/Generate_Sensing_Matrix.m:85-122
 *                            ('Random_Phase_State') and
 *                            generate_measurement/Generate_Measurement.m:67-136.
 *  ace_stage_host         <- test entry: one kernel of the r-column stages and of the pipeline around
 *                            them (init :296-310, ArgMinY :511-533, opt_X / opt_Y :384-385, the
 *                            rotation :263-264, quality :68, best of restarts :79-83, rollback and
 *                            rescale :93-107, the per-realisation partitions' Schur form) on host arrays.
 *  ace_nms_host           <- test entry: one operation of the A2nuclear m-space iteration (init, one
 *                            iteration, the pending convergence tests, the output parts) on host arrays.
 *  ace_pc_host            <- test entry: one operation of the private code-image kernels (code images, I + K,
 *                            the inverse, the tiles, A X0, one iteration launch) on host arrays.
 *  ace_pl_host            <- test entry: one operation of the PhaseLift step kernels (each step of the TFOCS
 *                            iteration, its GEMMs, the Cholesky setup, the final vector) on host arrays.
 *  ace_unit_host          <- test entry: one launch of the unit path's fused iteration kernels (gyk, gyf, the fused
 *                            apply_AH, the m-space run, its readiness count, opt_X from m-space) on host arrays.
 *
 * Conventions
 *  - Complex values are complex128, interleaved (re, im) doubles.
 *  - A is row-major [a_shared ? 1 : batch][m][n]; n = tx*rx with the
 *    column-major vec(H) ordering of the reference (element k = i + tx*j).
 *  - Per-realisation vectors are realisation-major: B[batch][m] (f64),
 *    X0/X[batch][n] (c128), Y[batch][m] (c128).
 *  - All pointers passed to ace_admm_solve_batch / ace_synth_* are DEVICE
 *    pointers; the caller owns every buffer (no allocation crosses the ABI).
 *  - Workspaces (every `workspace` / `workspace_bytes` pair): DEVICE memory of at least the matching
 *    *_workspace_size() bytes.  It may start at any address: every entry rounds the base up to 256 B before it
 *    carves, and every size query already includes that slack.  An entry reads nothing from its workspace that it has
 *    not written in the same call, so the contents on entry do not matter (tests/test_gpu_arena.py).
 *  - `stream` is a hipStream_t (NULL = default stream).  Calls are
 *    asynchronous on that stream except where noted; they are re-entrant per
 *    stream (no global mutable state besides the thread-local error text).
 *  - Return value 0 = success, negative = error; ace_last_error() returns a
 *    thread-local description of the last error on this thread.
 */
#ifndef ACE_H_
#define ACE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACE_OK 0
#define ACE_ERR_ARG -1        /* invalid argument / shape */
#define ACE_ERR_UNSUPPORTED -2 /* configuration outside the implemented scope */
#define ACE_ERR_HIP -3        /* HIP runtime error */
#define ACE_ERR_WORKSPACE -4  /* workspace too small */

#define ACE_VARIANT_A2ONLY 0  /* inferLowRankV4_multi.m ArgMinZ (rank-profile tail rescale) */
#define ACE_VARIANT_NUCLEAR 1 /* inferLowRank_Nuclear.m ArgMinZ (singular-value soft threshold) */

/* status bits per realisation */
#define ACE_ST_CONVERGED 1u   /* convergence test (inferLowRankV4_multi.m:372) passed */
#define ACE_ST_NO_OPT 2u      /* objective never finite: returned last iterate (reference would raise) */
#define ACE_ST_EIG_NOCONV 4u  /* Z-prox Jacobi hit its sweep cap at least once */
#define ACE_ST_ROLLBACK 8u    /* pipeline: refinement rolled back to X_max (inferLowRankV4_multi.m:94-98) */
#define ACE_ST_RANK_ONE 128u  /* pipeline: the last restart ran the rank-one retry (:73-77), so the refinement
                                 (:92/:100) uses the [1]/[0.95] profile -- set with stop_before_refine too, so a
                                 caller can hand the refinement's flags to ace_admm_cfg::rank_one */

typedef struct ace_admm_cfg {
    int variant;       /* ACE_VARIANT_* */
    int scale_by_row;  /* 1: row-wise magnitude step (:300-308, :344-351); 0: per-column (:352-361).  The two
                          coincide at r = 1 */
    int use_rank_one;  /* ArgMinZ rank profile [1] / [0.95] (inferLowRankV4_multi.m:448-450) for every
                          realisation, unless rank_one is given */
    int maxiter;       /* 500 in the reference (:13) */
    int fixed_iters;   /* 1: throughput mode -- run exactly maxiter iterations (no early exit) */
    int a_shared;      /* 1: one A for the whole batch (shared codebook); 0: private A per realisation */
    int eig_warm;      /* 1: warm-start the Z-prox Jacobi from the previous iteration's eigenvectors */
    int f64_applies;   /* 0: a shared phase-code A (every component in {0, +-c}) runs A v, A^H g and K Y
                          as exact int8 digit-plane products (f64 accuracy); 1: f64 matrix cores always */
    double mu0;        /* 1e-3   (:7) */
    double rho;        /* 1.03   (:8) */
    double tol_rel;    /* 1e-4   (:10) */
    double tol_abs;    /* 1e-8   (:11) */
    int r;             /* columns of X0: 1 (0 = 1) is the refinement stage (:92/:100); up to 32 on a shared A
                          (a_shared = 1): the r-column stages of inferLowRankImpl (:258 row-scaled, :270
                          per-column) */
    int reserved;
    /* Per-realisation use_rank_one [batch] (0/1 bytes, in the same memory space as the solve's other
     * buffers: device for ace_admm_solve_batch, host for ace_admm_solve_host), or NULL: use_rank_one for
     * every realisation.  The refinement of a batch of inferLowRankV4_multi calls passes each call's own
     * last-restart flag (:73-77, :92/:100): ACE_ST_RANK_ONE of ace_pipeline_solve_batch. */
    const uint8_t* rank_one;
} ace_admm_cfg;

/* Fill cfg with the reference defaults (inferLowRankV4_multi.m:6-14), variant A2only,
 * refinement stage (r = 1, scale_by_row = 1), shared A, convergence enabled. */
void ace_admm_cfg_default(ace_admm_cfg* cfg);

/* Workspace bytes needed by ace_admm_solve_batch for this problem (cfg->r columns). */
size_t ace_admm_workspace_size(const ace_admm_cfg* cfg, int batch, int m, int n);

/* Batched InferADMM on device buffers (r = cfg->r columns; R = scale_by_row ? r : 1 output columns).
 *   A      [a_shared?1:batch][m][n] c128      sensing matrix (codebook rows)
 *   B      [batch][m] f64                     RSS magnitudes
 *   X0     [batch][r][n] c128                 initial iterate (column j of realisation b contiguous)
 *   X, Y   [batch][R][n] / [batch][R][m] c128 out  best-objective iterate (opt_X, opt_Y; per-column mode
 *                                             returns the best column, :352-361)
 *   iters  [batch] int32 out (may be NULL)    iterations run
 *   status [batch] uint32 out (may be NULL)   ACE_ST_* bits
 *   mu     [batch] f64 out (may be NULL)      final penalty mu
 * Constraints: n == tx*rx, tx <= 32, rx <= 32 (tx, rx in {4,8,16,32} in the reference; A2only
 * with an odd tx <= 31 is solved as the zero-padded (tx + 1) x rx problem in buffers of its own,
 * `workspace` unused, and returns synchronously), m >= 1, 1 <= r <= 32 (r > 1: shared A only).
 * Returns once all kernels are enqueued; in convergence mode (fixed_iters == 0) the host polls a
 * device flag every few iterations and so synchronises `stream` periodically. */
int ace_admm_solve_batch(const ace_admm_cfg* cfg, int batch, int m, int n, int tx, int rx,
                         const double* A, const double* B, const double* X0,
                         double* X, double* Y, int32_t* iters, uint32_t* status, double* mu,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Host-pointer convenience wrapper: allocates device memory, copies in, solves,
 * copies out, frees.  Synchronous. */
int ace_admm_solve_host(const ace_admm_cfg* cfg, int batch, int m, int n, int tx, int rx,
                        const double* A, const double* B, const double* X0,
                        double* X, double* Y, int32_t* iters, uint32_t* status, double* mu);

/* ---- full recovery pipeline (inferLowRankV4_multi / inferLowRankV4 / inferLowRank_Nuclear) ----
 * MATLAB's randsample (:48), drawn inside every call, is replaced by train partitions: train_idx is a
 * HOST array of 0-based row indices, m_t = floor(m * cc_frac) per restart, in one of two layouts
 * (ace_pipeline_cfg::train_layout):
 *   ACE_TRAIN_SHARED          [restarts][m_t], one partition per restart for the whole batch;
 *   ACE_TRAIN_PER_REALISATION [batch][restarts][m_t], each realisation its own (a Monte-Carlo batch
 *                             of calls, each drawing its own randsample).
 * train_idx = NULL draws per-realisation partitions with the build's counter RNG from
 * ace_pipeline_cfg::train_seed (randperm prefixes, stream b * restarts + restart); it needs
 * train_layout = ACE_TRAIN_PER_REALISATION (ACE_ERR_ARG otherwise: the workspace size follows the layout).  Test rows are the
 * sorted complement (setdiff, :49).  Per-realisation partitions keep the stage state in m-space on the
 * full A (test rows held at zero) and apply (I + K_t)^{-1} through the full (I + K)^{-1} and a
 * per-realisation m_te x m_te block (the Schur identity; m - m_t <= 96, ACE_ERR_UNSUPPORTED beyond: the
 * Python mirror then solves the groups of realisations that share their partitions one call each);
 * realisations whose partitions coincide for every restart take the shared-A_t path.
 * Per realisation, stage_iters holds 4*restarts + 1 counts: for each restart the two
 * inferLowRankImpl stages (:258, :270), then the two stages of the rank-one retry (:73-77;
 * 0 when not run), then the refinement (:92/:100) -- the order of the oracle's stage_iters. */
typedef struct ace_pipeline_cfg {
    int variant;       /* ACE_VARIANT_A2ONLY (keep best restart) or ACE_VARIANT_NUCLEAR (last restart) */
    int restarts;      /* 3 (inferLowRankV4_multi.m:42), 1 (inferLowRankV4, inferLowRank_Nuclear) */
    int r;             /* 20 (:7); clipped to min(r, m, n) (:19), must be <= 32 */
    int maxiter;       /* 500 (:13), every stage */
    int eig_warm;      /* warm-start the Z-prox eigensolver inside each stage */
    int stop_before_refine; /* 0 (reference); 1: return X_max, the refinement's input (:90-92), rescaled
                          (:106-107), with Y_max on the train rows and no refinement stage (its
                          stage_iters column is 0) -- for measuring the unit on the reference's input */
    int train_layout;  /* ACE_TRAIN_SHARED (default) or ACE_TRAIN_PER_REALISATION (see above) */
    int train_seed;    /* seed of the build's draws when train_idx is NULL */
    double mu0;        /* 1e-3 */
    double rho;        /* 1.03 */
    double cc_frac;    /* 0.95 (:10) */
    double tol_rel;    /* 1e-4 */
    double tol_abs;    /* 1e-8 */
} ace_pipeline_cfg;

#define ACE_TRAIN_SHARED 0
#define ACE_TRAIN_PER_REALISATION 1
/* Reference defaults for `variant`: A2only -> 3 restarts, nuclear -> 1 restart. */
void ace_pipeline_cfg_default(ace_pipeline_cfg* cfg, int variant);
/* Workspace bytes for ace_pipeline_solve_batch (0 on invalid arguments).  Not monotonic in batch: a batch
 * of at most 16 realisations runs its restarts concurrently on one workspace copy each, so it can need
 * more than a batch of 17 -- size the workspace for the batch actually passed. */
size_t ace_pipeline_workspace_size(const ace_pipeline_cfg* cfg, int batch, int m, int n);
/* Batched pipeline on device buffers (shared codebook A [m][n] c128, B [batch][m] f64).
 * Outputs: X [batch][n], Y [batch][m] (c128; Y's last m - m_t entries are 0 after a
 * rollback, whose Y_max lives on the train rows), quality [batch] (the LAST restart's, as
 * the reference returns), stage_iters [batch][4*restarts+1], status [batch] (ACE_ST_*).
 * quality, stage_iters and status may be NULL.  Synchronises `stream` once per restart
 * (the rank-one retry set is decided on the host). */
int ace_pipeline_solve_batch(const ace_pipeline_cfg* cfg, int batch, int m, int n, int tx, int rx,
                             const double* A, const double* B, const int32_t* train_idx_host,
                             double* X, double* Y, double* quality, int32_t* stage_iters, uint32_t* status,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same on host arrays (allocates, copies, solves, frees; synchronous). */
int ace_pipeline_solve_host(const ace_pipeline_cfg* cfg, int batch, int m, int n, int tx, int rx,
                            const double* A, const double* B, const int32_t* train_idx,
                            double* X, double* Y, double* quality, int32_t* stage_iters, uint32_t* status);

/* ---- SpectralInitialize (inferLowRankV4_multi.m:561-574) ----------------------------------
 *   X = SpectralInitialize(A, B, r)
 * for a batch of magnitude vectors B [batch][m] (f64) sharing one A [m][n] (c128, row-major,
 * HOST arrays): X [batch][r][n] c128, column k = sqrt(s_k) v_k for the k-th largest eigenpair of
 * As^H As (As = rows of A scaled by B_i/||a_i||); eigenvectors are defined up to a unit phase
 * (MATLAB's eig and LAPACK pick one; the GPU picks another).  The pipeline's own initialisation
 * (ace_pipeline_solve_batch, :58) runs the same kernels: through the m x m dual Gram when m <= n,
 * the n x n primal Gram otherwise.  status [batch] (may be NULL): ACE_ST_EIG_NOCONV bits.
 * Synchronous; allocates its own device memory. */
int ace_spectral_init_host(int batch, int m, int n, int r, const double* A, const double* B, double* X,
                           uint32_t* status);

/* ---- PhaseLift (MyPhaseLift.m:69-107 via TFOCS solver_TraceLS / tfocs_AT) ----------------
 *   recoveredSig = MyPhaseLift(measurements, measurementMat)
 *   main/src/my_recovery_algorithms/MyPhaseLift.m:69 (called by Recover_Channel.m:34 with
 *   measurements = (rss/2e5).^2*1e10).  A batch of measurement vectors b [batch][m] sharing one
 *   measurement matrix Phi [m][n] (c128, row-major, DEVICE pointers); sig [batch][n] c128 out.
 *   The iteration runs in the coordinates of range(Phi^H) (exact for MyPhaseLift's zero start);
 *   m <= n needs full row rank (else ACE_ERR_UNSUPPORTED).  status: ACE_ST_CONVERGED when the
 *   TFOCS step tolerance stopped the run before maxIts. */
typedef struct ace_phaselift_cfg {
    int maxIts;        /* 4000 (MyPhaseLift.m:82) */
    int restart;       /* 200  (:84) */
    int cntr_reset;    /* 50   (tfocs_initialize.m; 10 when tol < 1e-12) */
    int reserved;
    double tol;        /* 1e-10 (:83), stopCrit 1 */
    double lambda;     /* 5e-2  (:91) */
    double L0, alpha, beta;  /* 1, 0.9, 0.5 (tfocs_initialize.m defaults) */
} ace_phaselift_cfg;
void ace_phaselift_cfg_default(ace_phaselift_cfg* cfg);
size_t ace_phaselift_workspace_size(const ace_phaselift_cfg* cfg, int batch, int m, int n);
int ace_phaselift_solve_batch(const ace_phaselift_cfg* cfg, int batch, int m, int n, const double* Phi,
                              const double* b, double* sig, int32_t* iters, uint32_t* status,
                              void* workspace, size_t workspace_bytes, void* stream);
int ace_phaselift_solve_host(const ace_phaselift_cfg* cfg, int batch, int m, int n, const double* Phi,
                             const double* b, double* sig, int32_t* iters, uint32_t* status);
/* ace_phaselift_solve_host plus solver_TraceLS's result itself (MyPhaseLift.m:98 recoveredMat, the final
 * tfocs_AT iterate): Xr [batch][d][d] c128 (HOST), d = min(m, n), in the coordinates of range(Phi^H)
 * (recoveredMat = Q Xr Q^H, Phi^H = Q R with R = chol(Phi Phi^H); Q = I when m > n).  For parity tests of the
 * iterate and of the TFOCS objective 0.5 ||A(X) - b||^2 + lambda tr X. */
int ace_phaselift_solve_host_x(const ace_phaselift_cfg* cfg, int batch, int m, int n, const double* Phi,
                               const double* b, double* sig, int32_t* iters, uint32_t* status, double* Xr);
/* The prox's eigensolver alone (prox_trace.m:88-92: all eigenpairs of a Hermitian d x d matrix above tau),
 * for parity tests of its paths: A [batch][d][d] c128 (HOST, Hermitian; the lower triangle is read), tau [batch];
 * lam [batch][d] (descending; entries >= k[b] undefined), V [batch][d][d] c128 (eigenvector q as row q),
 * k [batch].  path: 0 unblocked one-stage, 1 blocked one-stage, 2 two-stage (where it applies, else 1); + 4: the
 * vectors of the smaller side of tau (PhaseLift's ACE_PROX_SIDE=1): when more than half of the eigenvalues exceed
 * tau, V holds those at or below it (ascending) and k[b] = -(their count).
 * Synchronous; allocates its own device memory. */
int ace_prox_eig_host(int batch, int d, int path, const double* A, const double* tau, double* lam, double* V,
                      int32_t* k);

/* ---- test entries: one application of a linear operator of the ADMM iteration ---------------
 * The four operators every solver loops around, on their own (tests/test_gpu_linops.py compares them with
 * exact references):
 *   ACE_LINOP_A      T  = (Y - M/mu) - A (Z - N/mu)
 *   ACE_LINOP_AH     X  = (Z - N/mu) + A^H g     (ACE_LINOP_I8 at rcols = 1: W = A^H g alone, as the Z-step takes it)
 *   ACE_LINOP_K      KY = K g,  K = A A^H        (the operand is passed in `g`)
 *   ACE_LINOP_G      g' = G g,  G = (I + K)^-1   (the operand is passed in `g`; f64 only)
 *   ACE_LINOP_SETUP  no application: out = K, out2 = G ([1 | batch][m][m] c128) and out3 = {c, c^2} (the
 *                    phase-code scale; zeros unless path = ACE_LINOP_I8) as the operator setup left them
 * The entry builds the operators with the solver's own setup, fills one control block per realisation from
 * mu / vbound / done / nzero / avok (every other field zero) and makes the launcher calls a solve makes for the
 * operator on the chosen path:
 *   ACE_LINOP_F64        a_shared: the pre-pass (V = Z - N/mu, S = Y - M/mu) and the 3M matrix-core GEMM;
 *                        private codebooks (a_shared = 0, rcols = 1): the pre-pass and the GEMV kernels
 *   ACE_LINOP_F64_FUSED  shared A, rcols = 1, A / AH: the GEMM with the pre-pass folded in
 *   ACE_LINOP_I8         shared phase-code A: the exact int8 digit planes (rcols = 1: the unit path's launches;
 *                        rcols > 1: the r-column stages', vector j of realisation j / rcols).  ACE_ERR_UNSUPPORTED
 *                        when the setup does not take the codebook (no fall-back to f64).
 * All arrays are HOST, row-major c128 as (re, im) doubles: A [1 | batch][m][n]; Z, N [batch * rcols][n];
 * Y, M, g, AX [batch * rcols][m]; mu, vbound, done, nzero, avok [batch].  N, M (NULL: zero), vbound (NULL: 0), the
 * flags (NULL: 0) and AX (int8 apply_A at rcols = 1 only: the A V of realisations with avok) are optional.
 * out ([batch * rcols][m], AH: [..][n]) is filled with `sentinel` before the launch, so rows a kernel leaves
 * alone (done realisations) show.  The fused kernels that carry solver state (the g / Y-step / K Y kernels, the
 * apply_AH's fused Z-step) are not reachable from here; the private code-image kernels (pgk_kernel and their setup)
 * are reachable one launch at a time through ace_pc_host below.
 * Synchronous; allocates its own device memory. */
#define ACE_LINOP_A 0
#define ACE_LINOP_AH 1
#define ACE_LINOP_K 2
#define ACE_LINOP_G 3
#define ACE_LINOP_SETUP 4
#define ACE_LINOP_F64 0
#define ACE_LINOP_F64_FUSED 1
#define ACE_LINOP_I8 2
typedef struct ace_linop_args {
    int op, path, a_shared, batch, m, n, rcols, reserved;
    const double* A;
    const double *Z, *N, *Y, *M, *g, *AX;
    const double *mu, *vbound;
    const int32_t *done, *nzero, *avok;
    double sentinel;
    double *out, *out2, *out3;
} ace_linop_args;
int ace_linop_host(const ace_linop_args* args);
/* The f64 3M matrix-core GEMM launcher with all of its arguments (test entry):
 *   C[z][b][i] = epi( sum_k op(L[z])[i][k] V[z][b][k] ),  mode 0: acc, 1: E - acc, 2: E + acc;  conj_l: op = conj.
 * L, V, C, E: HOST c128 arrays of nL, nV, nC, nC complex elements with leading dimensions ldl, ldv, ldc and z strides
 * (complex elements); C is uploaded as given (a caller's sentinel shows what the kernel wrote) and read back.  klim
 * (optional, nklim doubles): per z-slice bound on k, read from klim[z * klim_stride]; the operands must be zero at
 * and beyond it.  ACE_ERR_ARG when an operand extent exceeds its array.  Synchronous. */
int ace_zgemm_host(int mode, int conj_l, int M, int K, int nb, const double* L, long long nL, int ldl, long long strideL,
                   const double* V, long long nV, int ldv, long long strideV, double* C, const double* E, long long nC,
                   int ldc, long long strideC, int nz, const double* klim, long long nklim, long long klim_stride);

/* ---- test entry: one Z-step (ArgMinZ, the N update and the iteration control) on host arrays --------
 * The other half of every ADMM iteration on its own (tests/test_gpu_zprox.py compares it with an
 * extended-precision transcription of inferLowRankV4_multi.m:423-485 and :344-381).  The entry fills a Z-step
 * argument block and one control block per realisation the way a solve does and calls the solve's Z-step
 * launcher (init != 0: its init form, mu = 1, N = 0, no iteration control), preceded by the lean steady-state
 * kernel when lean != 0.  Which kernel runs follows the solver's rule: the one-wave kernel at r = 1, the
 * four-wave kernel otherwise.
 *   variant      ACE_VARIANT_A2ONLY | ACE_VARIANT_NUCLEAR
 *   tx, rx, r    the iterate of a realisation is [r][n], n = tx rx, each column a tx x rx matrix (column-major);
 *                2 <= tx <= 32 even (the API pads odd tx), 1 <= rx <= 32, 1 <= r <= 32
 *   m            rows of the thresholds (:364-370) and of rank_profile
 *   np, rl, fl   the rank profile; np = 0: rank_profile(tx, rx, m, n, 0)
 *   rank_one     (optional) [batch] per-realisation use_rank_one: profile [1] / [0.95]
 *   row_mode     scale_by_row (r > 1; r = 1 runs as row mode)
 *   it           the iteration being controlled (>= 1; init: ignored)
 *   warm, tkeig, r1lz, zcert   the path switches of the Z-step argument block, passed through
 *   wmode        r = 1, not init: X holds W = A^H g and the kernel forms X = (Z - N/mu) + W; needs pingpong
 *   pingpong     Z', N' go to buffers of their own (wmode only), which start from `sentinel`
 *   lean         the lean kernel first (A2only, r = 1, wmode, warm, n a multiple of 64 else it is a no-op)
 * Inputs (HOST, c128 as (re, im) doubles): X [batch][r][n]; Z, N [batch][r][n] (NULL: zero; init ignores them);
 * Q [batch][tx][tx] warm-start eigenvectors (NULL: the buffer starts from `sentinel`; required when warm and not
 * init); state [batch][ACE_ZP_NIN] doubles and flags [batch][ACE_ZP_NFLAG] int32 (either NULL: zeros, mu = 1),
 * every control-block field not listed there is zero:
 *   state: mu, last_res, opt_obj, obj2, nAX2, nY2, nJM2, dY2, dAtY, nAtY, kfcum, kf[0..3]
 *   flags: done, nzero, kfok, optsrc
 * The Y-step sums and the dual terms are the caller's numbers (the r = 1 kernel takes them as the fused Y-step
 * kernel leaves them; the four-wave kernel forms the dual terms itself from Y and K Y buffers, which are zero
 * here: dAtY = nAtY = 0 there).
 * Outputs (HOST; each may be NULL): Zo, No [batch][r][n] (in place: the Z, N buffers after the step); Qo
 * [batch][tx][tx]; optX, Xcur [batch][row_mode ? r : 1][n] (both start from `sentinel`);
 *   state_out [batch][ACE_ZP_NOUT]: mu, last_res, opt_obj, vbound, kf[0..3], kfcum
 *   flags_out [batch][ACE_ZP_NFLAGOUT]: iters, done, status, nzero, avok, kfok, optsrc, zit
 *   tkcnt [2]: top-K tridiagonal uses and fallbacks to the Jacobi eigensolver
 * ACE_ERR_ARG: bad shapes or missing arrays; ACE_ERR_UNSUPPORTED: a combination no solve makes (wmode without
 * pingpong or at r > 1 or in the init form, pingpong without wmode, lean outside its conditions, odd tx).  The
 * producers of the Z-step's inputs that carry solver state (the fused apply_AH, the A2only m-space steady state
 * and the compact launch) are not reachable from here; the A2nuclear m-space state and its lazy dual residual
 * are reachable through ace_nms_host below.
 * Synchronous; allocates its own device memory. */
#define ACE_ZP_NIN 15
#define ACE_ZP_NFLAG 4
#define ACE_ZP_NOUT 9
#define ACE_ZP_NFLAGOUT 8
typedef struct ace_zprox_args {
    int variant, batch, tx, rx, r, m;
    int np, rl[4];
    double fl[4];
    int init, row_mode, it, fixed_iters;
    int warm, tkeig, r1lz, zcert, wmode, pingpong, lean, reserved;
    double tol_rel, tol_abs, rho, sentinel;
    const unsigned char* rank_one;
    const double *X, *Z, *N, *Q, *state;
    const int32_t* flags;
    double *Zo, *No, *Qo, *optX, *Xcur, *state_out;
    int32_t *flags_out, *tkcnt;
} ace_zprox_args;
int ace_zprox_host(const ace_zprox_args* args);

/* ---- test entry: one kernel of the r-column stages / of the pipeline around them on host arrays --------
 * The kernels of csrc/ace_stage.hip on their own (tests/test_gpu_stage.py compares them with longdouble
 * transcriptions of inferLowRankV4_multi.m, tests/stage_ref.py).  The entry uploads the operands, fills every output
 * with `sentinel` (int32 outputs: `isentinel`, byte outputs: its low byte), fills one control block per realisation
 * from state / flags where the kernel reads one (every other field zero; both NULL: zeros, mu = 1) and calls the
 * launcher a solve calls.  All arrays are HOST; c128 as (re, im) doubles.  Outputs may be NULL.
 *   state [batch][ACE_SG_NSTATE]: mu, last_res, opt_obj, nB, obj2, nAX2, nY2, nJM2, dY2
 *   flags [batch][ACE_SG_NFLAG]:  iters, done, status, objcol, optsrc, optysrc
 * op (sizes; inputs -> outputs):
 *   INIT_R       row_mode, batch, n, m, r, mu0; X (X0) [b][r][n], P0 (= A X0) [b][r][m], B [b][m], mask [b][m]
 *                (optional, 1 on train rows) -> Xo, No [b][r][n], Yo, Mo [b][r][m], state_out, flags_out
 *   YSTEP_R      row_mode, batch, m, r; S, g, M, Y (Y_old) [b][r][m], B, mask, state (mu), flags (done)
 *                -> Yo (Y_new), Mo (M in place), state_out, flags_out
 *   FINALIZE_R   batch, n, m, r, nc; optX [b][nc][n], optY [b][nc][m], X (current) [b][r][n], Y [b][r][m], Zb1, Zb2,
 *                Yb1, Yb2 (optional, as optX / optY), state, flags -> Xo [b][nc][n], Yo [b][nc][m], qo [b] (mu),
 *                iout [b][2] (iters, status)
 *   GRAM_ROTATE  batch, n, r; X [b][r][n], idst [b] (optional status in) -> Xo, iout [b] (status)
 *   QUALITY      batch, n, count (= m_te, may be 0); A [count][n], X [b][n], B [b][count] -> qo [b]
 *   PART_QUALITY batch, n, m, mt; A [m][n], X [b][n], B [b][m], rows [b][m] -> qo [b]
 *   KEEP_BEST    batch, n, m, first; q, qmax [b], X [b][n], Y [b][m], Xmax, Ymax (optional: sentinel)
 *                -> qo (qmax), Xo (Xmax), Yo (Ymax)
 *   FINISH       batch, n, m, mt; q (last quality) [b], X [b][n], Y [b][m], Xmax [b][n], Ymax [b][mt], anorm [1],
 *                bnorm [b], idst [b] (optional status in) -> Xo [b][n], Yo [b][m], iout [b] (status)
 *   PART_GEINV   batch, m, mt; G [m][m], rows, idst (optional status in) -> Xo [b][te][te], iout [b] (status)
 *   PART_GFIX    batch, m, mt, r; G, geinv [b][te][te], g (= G T~) [b][r][m], rows, mask [b][m], flags (optional: done)
 *                -> Yo [b][r][m] (g in place)
 *   PART_EXPAND  batch, m, mt, r; Y [b][r][mt], rows -> Yo [b][r][m];  PART_COMPACT the other way
 *   ANORM        m, n, tol_abs; A [m][n] -> qo [1]
 *   BNORM        batch, m, tol_abs; B [b][m] -> qo [b] (B_norm), Xo [b][m] doubles (B / B_norm)
 *   GATHER_ROWS  m, n, count; A [m][n], idx [count], anorm [1] -> Xo [count][n]
 *   GATHER_B     batch, m, count; B [b][m], idx [count] -> qo [b][count]
 *   MOVE_ROWS    count, len, m, scatter; src [scatter ? count : m][len] doubles, idx [count] (into the m rows of the
 *                other side) -> qo [scatter ? m : count][len];  MOVE_BYTES the same on bsrc -> bout
 *   PUT_COL      count, m, ld, col, or_mask; isrc [count], idx (optional, distinct), idst [m][ld] (optional) -> iout
 *   FLAG_BITS    count, m, bit; bsrc [count] flags, idst [m] (optional) -> iout [m]
 *   FILL         len, m, value -> qo [m] (the first len elements)
 * Checked before any HIP call, with the argument's name in ace_last_error(): ACE_ERR_ARG for a NULL array, a size
 * out of range, rows that are no permutation of 0 .. m-1 or an idx outside its array; ACE_ERR_UNSUPPORTED for
 * r > 32 and for m - mt > 96 test rows.  Synchronous; allocates its own device memory. */
enum {
    ACE_STAGE_INIT_R = 0, ACE_STAGE_YSTEP_R, ACE_STAGE_FINALIZE_R, ACE_STAGE_GRAM_ROTATE, ACE_STAGE_QUALITY,
    ACE_STAGE_PART_QUALITY, ACE_STAGE_KEEP_BEST, ACE_STAGE_FINISH, ACE_STAGE_PART_GEINV, ACE_STAGE_PART_GFIX,
    ACE_STAGE_PART_EXPAND, ACE_STAGE_PART_COMPACT, ACE_STAGE_ANORM, ACE_STAGE_BNORM, ACE_STAGE_GATHER_ROWS,
    ACE_STAGE_GATHER_B, ACE_STAGE_MOVE_ROWS, ACE_STAGE_MOVE_BYTES, ACE_STAGE_PUT_COL, ACE_STAGE_FLAG_BITS,
    ACE_STAGE_FILL, ACE_STAGE_NOPS
};
#define ACE_SG_NSTATE 9
#define ACE_SG_NFLAG 6
typedef struct ace_stage_args {
    int32_t op, row_mode, batch, n, m, r, nc, mt;
    int32_t count, ld, col, first, scatter, isentinel;
    uint32_t or_mask, bit;
    int64_t len;
    double mu0, tol_abs, value, sentinel;
    const double *X, *Y, *P0, *B, *S, *g, *M, *A, *G, *geinv;
    const double *q, *qmax, *Xmax, *Ymax, *anorm, *bnorm, *optX, *optY, *Zb1, *Zb2, *Yb1, *Yb2, *src;
    const double* state;
    const int32_t* flags;
    const int32_t *rows, *idx, *isrc, *idst;
    const unsigned char *mask, *bsrc;
    double *Xo, *Yo, *Mo, *No, *qo, *state_out;
    int32_t *iout, *flags_out;
    unsigned char* bout;
} ace_stage_args;
int ace_stage_host(const ace_stage_args* args);

/* ---- test entry: one operation of the A2nuclear m-space iteration (csrc/ace_nucmsp.hip) on host arrays --------
 * The benchmarked inner loop of the A2nuclear r = 1 solve on its own (tests/test_gpu_nms.py compares it with the
 * references of tests/nms_ref.py).  The entry fills the kernel's argument blocks and one control block per
 * realisation the way the solve does (lazy dual residual, r = 1) and calls the solve's launcher:
 *   ACE_NMS_INIT  Xinit [b][n], P0 = A X_init [b][m] -> Eo_out (zeros), AEo_out (= P0), state_out (na, naz, nbeta,
 *                 nep2, nx0, nopt_a, ncur_a), flags_out (dpend)
 *   ACE_NMS_STEP  the dense G = (I + K)^-1 and K = A A^H [m][m] are packed in matrix-core fragment order, then one
 *                 iteration `it` (>= 1): Yo (Y of the previous iterate), M, B [b][m] doubles, Eo, AEo, state, flags;
 *                 Yn (the iterate before Yo) is read only where a convergence test is pending (flags dpend)
 *                 -> Yn_out (Y_new), M_out, En_out, AEn_out, optW_out, optY_out, curW_out, state_out, flags_out
 *   ACE_NMS_FIN   only the convergence tests left pending: K, Yo, Yn, state, flags -> state_out, flags_out
 *   ACE_NMS_OUT   Xinit, state (opt_obj, nopt_a, ncur_a), optW, curW -> V [b][n] (the X_init part of the selected
 *                 iterate), Wsel [b][m] (its m-part; the caller adds A^H Wsel)
 * All arrays are HOST; c128 as (re, im) doubles.  A per-realisation vector array the caller leaves NULL starts from
 * `sentinel` on the device, En / AEn / V / Wsel always do, and every one of them is followed by `guard` doubles of
 * `sentinel`: an output array has its rows and then the guard, so untouched memory can be asserted.  The arrays a
 * kernel must not write (B, Yo, Eo, AEo) come back as well.  Outputs may be NULL.
 *   state, state_out [batch][ACE_NMS_NSTATE]: mu, last_res, opt_obj, na, naz, nbeta, nep2, nopt_a, ncur_a, pd_dZ2,
 *          pd_nZ2, pd_rc, obj2, nAX2, nY2, nJM2, dY2, dAtY, nAtY, nx0   (NULL state: zeros, mu = 1)
 *   flags, flags_out [batch][ACE_NMS_NFLAG]: iters, done, status, dpend
 *   done_count / done_count_out: the batch's count of stopped realisations before / after
 *   guard_ok: 1 when the control block after the batch's and every control-block field not listed above are as
 *          they were
 * The state passes through exactly, so a caller chains init, steps, fin and out by handing the outputs back with
 * the ping-pong pairs (Yo / Yn, Eo / En, AEo / AEn) swapped.
 * Checked before any HIP call: ACE_ERR_ARG for an unknown op, batch, n or m < 1, a negative guard, rho <= 0
 * (step, fin), it < 1 (step) and a NULL required array (named in ace_last_error()); ACE_ERR_UNSUPPORTED for
 * m > 256 and for a refused LDS request.  Synchronous; allocates its own device memory. */
enum { ACE_NMS_INIT = 0, ACE_NMS_STEP, ACE_NMS_FIN, ACE_NMS_OUT, ACE_NMS_NOPS };
#define ACE_NMS_NSTATE 20
#define ACE_NMS_NFLAG 4
typedef struct ace_nms_args {
    int32_t op, batch, n, m, it, fixed_iters, guard, done_count;
    double tol_rel, tol_abs, rho, sentinel;
    const double *Xinit, *P0, *G, *K, *B, *Yo, *Yn, *M, *Eo, *AEo, *optW, *optY, *curW, *state;
    const int32_t* flags;
    double *B_out, *Yo_out, *Yn_out, *M_out, *Eo_out, *En_out, *AEo_out, *AEn_out, *optW_out, *optY_out, *curW_out;
    double *V, *Wsel, *state_out;
    int32_t *flags_out, *done_count_out, *guard_ok;
} ace_nms_args;
int ace_nms_host(const ace_nms_args* args);

/* ---- test entry: one operation of the private code-image kernels (csrc/ace_private.hip) on host arrays --------
 * The setup and iteration kernels of the private phase-code path (one codebook per realisation) on their own
 * (tests/test_gpu_pc.py compares them with the references of tests/pc_ref.py).  Every operation calls the launchers
 * a solve calls; launch_pc_ginv's three steps are reachable one at a time:
 *   ACE_PC_PACK     A [b][m][n] -> cb [b], flag_out [1], codes (the A^H, A and row-major images of the batch, one
 *                   after the other as the launcher lays them out: b nH, b nA, b nR dwords)
 *   ACE_PC_KMAT     A (packed first) -> Gw [b][mp32][mp32] = I + K (pc_k_kernel alone)
 *   ACE_PC_INV      Gin [b][mp32][mp32] Hermitian positive definite, form (ACE_PC_SCHUR / ACE_PC_GJ) -> Gw, the
 *                   inverse in place (the inverse launcher alone)
 *   ACE_PC_TILES    Gin [b][mp32][mp32] -> Gt [b][ntile][16][16] (pc_tiles_kernel alone)
 *   ACE_PC_APPLY_A  A (packed first), X0 [b][n] -> P0 [b][m]
 *   ACE_PC_STEP     one pgk_kernel launch: A (packed first); G [b][m][m] (NULL: the setup's own G_b through
 *                   launch_pc_ginv; given: through pc_tiles_kernel, only its lower 16 x 16 tiles are read); B [b][m]
 *                   doubles, Yo, M [b][m], Z, N [b][n], state, flags; AX, Yn, optY [b][m] optional (NULL: sentinel);
 *                   yn_id 0 (opt_Y copied at once) or 1 / 2 (deferred, RealState::optysrc)
 *                   -> AX_out, M_out, Yn_out, W [b][n], optY_out, state_out, flags_out, Gt, and the arrays the
 *                   kernel must not write (B_out, Yo_out, Z_out, N_out)
 * mp32 = 32 ceil(m / 32), ntile = mt (mt + 1) / 2 with mt = ceil(m / 16); with nct = ceil(n / 16):
 * nH = nct ceil(mt / 8) 128, nA = mt ceil(nct / 8) 128, nR = m nct.
 * All arrays are HOST; c128 as (re, im) doubles.  Every device buffer a kernel writes starts from `sentinel` (the code
 * images: from 0xFF bytes) and is followed by `guard` doubles (dwords) of it: an output array has its rows and then
 * the guard (codes: one guard after the three images; Gw: the guard that follows the recursion's scratch).  Outputs
 * may be NULL.
 *   state, state_out [batch][ACE_PC_NSTATE]: mu, opt_obj, vbound, obj2, nAX2, nY2, nJM2, dY2, dAtY, nAtY
 *   flags, flags_out [batch][ACE_PC_NFLAG]: done, avok, nzero, optysrc
 *   guard_ok: 1 when the control block after the batch's and every control-block field not listed above are as
 *          they were
 * Checked before any HIP call: ACE_ERR_ARG for an unknown op or form, batch, m or n < 1, a negative guard, yn_id
 * outside 0..2, mu <= 0 (step) and a NULL required array (named in ace_last_error()); ACE_ERR_UNSUPPORTED for
 * m > 256, n > 2048 and for an LDS request beyond pc_supported.  Synchronous; allocates its own device memory. */
enum { ACE_PC_PACK = 0, ACE_PC_KMAT, ACE_PC_INV, ACE_PC_TILES, ACE_PC_APPLY_A, ACE_PC_STEP, ACE_PC_NOPS };
enum { ACE_PC_SCHUR = 0, ACE_PC_GJ, ACE_PC_NFORMS };
#define ACE_PC_NSTATE 10
#define ACE_PC_NFLAG 4
typedef struct ace_pc_args {
    int32_t op, form, batch, m, n, yn_id, guard, reserved;
    double sentinel;
    const double *A, *Gin, *X0, *G, *B, *Yo, *M, *AX, *Yn, *optY, *Z, *N, *state;
    const int32_t* flags;
    double* cb;
    uint32_t* codes;
    double *Gw, *Gt, *P0, *B_out, *Yo_out, *M_out, *AX_out, *Yn_out, *optY_out, *W, *Z_out, *N_out, *state_out;
    int32_t *flag_out, *flags_out, *guard_ok;
} ace_pc_args;
int ace_pc_host(const ace_pc_args* args);

/* ---- test entry: one operation of the PhaseLift step kernels (csrc/ace_phaselift.hip) on host arrays ------------
 * The kernels of the TFOCS Auslender-Teboulle iteration of MyPhaseLift, its setup and its output on their own
 * (tests/test_gpu_pl.py compares them with the restatements of tests/pl_ref.py).  Every operation calls the launcher
 * the solve calls (launch_pl_*, launch_chol, launch_ztranspose, and launch_zgemm through the solve's own pl_apply_A /
 * pl_g_y / pl_zasm):
 *   ACE_PL_INIT         pl_init_kernel: bvec -> gAy, gAx, state
 *   ACE_PL_OUTER_BEGIN  pl_outer_begin_kernel: x, z, Ax, Az, state -> xo, zo, Axo, Azo, state
 *   ACE_PL_THETA        pl_theta_kernel: state, cnt -> state, act, cnt
 *   ACE_PL_MAKE_Y       pl_make_y_kernel: xo, zo, state, act -> y
 *   ACE_PL_SET_AY       pl_set_Ay_kernel: Axo, Azo, Aex, state, act -> Ay
 *   ACE_PL_GRAD         pl_grad_kernel: Ay, bvec, gAy, R, state, act -> gAy, Pg, tau, state
 *   ACE_PL_GY           the solve's GEMM G = R diag(g) R^H: R, Pg -> G
 *   ACE_PL_PROX_IN      pl_prox_in_kernel: zo, G, state, act -> C
 *   ACE_PL_ASSEMBLE     pl_assemble_kernel: V, lam, misc, tau, state, act -> P, VT, state
 *   ACE_PL_ZASM         the solve's batched klim GEMM: VT, P, misc -> Znew
 *   ACE_PL_TAKE_Z       pl_take_z_kernel: Znew, zo, G, misc, tau, state, act -> z
 *   ACE_PL_APPLY_A      the solve's A(x): the RT GEMM, then pl_diagform_kernel: x, R, RT, act -> T, Aex
 *   ACE_PL_MAKE_X       pl_make_x_kernel: xo, z, y, G, Axo, Az, state, act, cnt -> x, Ax, state, cnt
 *   ACE_PL_SET_AX       pl_set_Ax_kernel: Aex, state, act -> Ax
 *   ACE_PL_BACKTRACK    pl_backtrack_kernel: Ax, Ay, bvec, gAy, state, act -> gAx, state
 *   ACE_PL_ITERATE      pl_iterate_kernel: x, Ax, gAx, state, cnt -> y, z, Ay, Az, gAy, state, cnt
 *   ACE_PL_CHOL         chol_kernel: K [m][m] -> cholR [m][m], ok [1]
 *   ACE_PL_TRANSPOSE    ztranspose_kernel: R [d][m] -> RT [m][d]
 *   ACE_PL_FINAL_VEC    pl_final_in_kernel, then pl_final_vec_kernel: x, V1 [b][d], lam (lam[b][0] is read), `reduced`
 *                       (1: R [d][d] upper triangular, m == d) -> C, w [b][d]
 *   ACE_PL_OUTPUTS      pl_outputs_kernel: state, status -> iters, status
 * Shapes (HOST arrays; c128 as (re, im) doubles): x, xo, z, zo, y, G, Znew, P, VT, V, C [b][d][d] c128; Ax, Axo, Az,
 * Azo, Ay, gAy, gAx, Aex, bvec [b][m] f64; R [d][m], RT [m][d] c128; Pg, T [b][d][m] c128; tau [b]; lam [b][d];
 * misc [b][3]; K, cholR [m][m] c128; V1, w [b][d] c128; act, iters, status [b], cnt [9], ok [1] int32.  C, lam and misc
 * are the eigensolver's slots of the scratch, at heev_layout(d, d) offsets (FINAL_VEC: heev_layout(d, 1)).
 * An input that is NULL starts from `sentinel` (int32: from ACE_PL_ISENTINEL); every buffer is followed by `guard`
 * doubles (ints) of it and comes back, guard included, in its `_out` array (count + guard elements; may be NULL).
 *   state, state_out [batch][ACE_PL_NSTATE]: L, L_old, theta, theta_old, f_x, f_y, C_x, C_z, cntr_Ax, cntr_Ay, xy_sq,
 *          nx2, ndx2, dot_xy_g, localL, step, n_iter, restart_iter, backtrack_simple, backtrack_steps, have_gAy,
 *          have_gy, have_gAx, ycomp, need_Ay, need_Ax, inner, done, status
 *          (PlState in field order; the int32 fields as exact doubles, Inf and NaN carried through)
 *   guard_ok: 1 when every guard, every buffer the operation does not write (the rest of the scratch and the state's
 *          padding included) and the state block after the batch's are bit for bit as they were
 * Checked before any HIP call: ACE_ERR_ARG for an unknown op, batch, m or d < 1, a negative guard, reduced with
 * m != d (FINAL_VEC) and a NULL required array (named in ace_last_error()); ACE_ERR_UNSUPPORTED for d > 1600.
 * Synchronous; allocates its own device memory. */
enum {
    ACE_PL_INIT = 0, ACE_PL_OUTER_BEGIN, ACE_PL_THETA, ACE_PL_MAKE_Y, ACE_PL_SET_AY, ACE_PL_GRAD, ACE_PL_GY,
    ACE_PL_PROX_IN, ACE_PL_ASSEMBLE, ACE_PL_ZASM, ACE_PL_TAKE_Z, ACE_PL_APPLY_A, ACE_PL_MAKE_X, ACE_PL_SET_AX,
    ACE_PL_BACKTRACK, ACE_PL_ITERATE, ACE_PL_CHOL, ACE_PL_TRANSPOSE, ACE_PL_FINAL_VEC, ACE_PL_OUTPUTS, ACE_PL_NOPS
};
#define ACE_PL_NSTATE 29
#define ACE_PL_ISENTINEL 0x5A5A5A5A
typedef struct ace_pl_args {
    int32_t op, batch, m, d, guard, reduced, cntr_reset, restart, maxIts, reserved;
    double lambda, alpha, beta, Lexact, tol, L0, sentinel;
    const double *x, *xo, *z, *zo, *y, *G, *Znew, *P, *VT, *V, *Ax, *Axo, *Az, *Azo, *Ay, *gAy, *gAx, *Aex, *bvec, *R, *RT;
    const double *Pg, *T, *tau, *C, *lam, *misc, *K, *cholR, *V1, *w, *state;
    const int32_t *act, *cnt, *ok, *iters, *status;
    double *x_out, *xo_out, *z_out, *zo_out, *y_out, *G_out, *Znew_out, *P_out, *VT_out, *V_out, *Ax_out, *Axo_out;
    double *Az_out, *Azo_out, *Ay_out, *gAy_out, *gAx_out, *Aex_out, *bvec_out, *R_out, *RT_out, *Pg_out, *T_out;
    double *tau_out, *C_out, *lam_out, *misc_out, *K_out, *cholR_out, *V1_out, *w_out, *state_out;
    int32_t *act_out, *cnt_out, *ok_out, *iters_out, *status_out, *guard_ok;
} ace_pl_args;
int ace_pl_host(const ace_pl_args* args);

/* ---- test entry: one launch of the unit path's fused iteration kernels (csrc/ace_i8gemm.hip) on host arrays -----
 * The kernels that iterate the A2only r = 1 solve on a shared phase-code A, one launcher call at a time
 * (tests/test_gpu_unit.py compares them with the references of tests/unit_ref.py).  The entry builds the operators
 * from A as a solve does (linops_carve / linops_setup with the int8 digit planes), fills GykArgs, ZArgs, DualCtl and
 * MsrArgs the way admm_iterate_split does at iteration `it` (ping-pong choices by it & 1 and q, yn_id = 2 - q,
 * Sold = S[(it + 1) & 1], Snew = S[it & 1], Z = (it & 1) ? Zb1 : Zb2 with the other buffer as Z', fixup_now =
 * (it == maxiter)), one control block per realisation from state / flags (every other field zero), and calls:
 *   ACE_UNIT_GYK    launch_gyk: T (use_la = 0: the caller's T; 1: apply_A folded in, from Z, N), g = G T, the Y-step
 *                   (Yo = Y[q] -> Yn = Y[1 - q], M in place, AX when use_ax), opt_Y (yn_copy = 1: yn_id = 0, copied);
 *                   lazy = 0: K Y' into KY[1 - q] and dAtY, nAtY; lazy = 1: none, pending tests finished first
 *   ACE_UNIT_GYF    launch_gyf (lazy, apply_A folded in, AX): the same body, the fused apply_AH pass into Z' (or W
 *                   into X), and with msp = 1 the m-space entry and steps; ctl = 1: fused_control in place
 *   ACE_UNIT_AHF    launch_i8_apply_AH with the fused epilogue (i8ah_kernel<false, true>), g from memory
 *   ACE_UNIT_MSR    launch_msr: iterations it .. it_end - 1 in one launch, `waves` 8 or 4 (m = 256 only)
 *                   -> resume [1], steps [4], mspcount_out, vecw [1]
 *   ACE_UNIT_READY  launch_msr_ready -> ready [3]
 *   ACE_UNIT_OPTX   launch_i8_msp_optx: optS (S0 / S1 where optsrc is 4 / 5), Zb1 / Zb2 by z0id -> optX
 * and hands back the f64 K, G [m][m] c128 and c8 = {c, c^2} the setup produced (K_out, G_out, c_out; may be NULL).
 * Per-realisation arrays (HOST; c128 as (re, im) doubles): B [b][m] f64; T, g, Y0, Y1, KY0, KY1, M, AX, optY, S0, S1,
 * optS [b][m] c128; Zb1, Zb2, Nb1, Nb2, X, Xcur, optX [b][n] c128.  One the caller leaves NULL starts from `sentinel`,
 * and each is followed by `guard` doubles of `sentinel`; each comes back, guard included, in its `_out` array (may be
 * NULL).  rank_one [b] bytes (may be NULL: the profile np, fl[] for every realisation).  The N of the previous iterate
 * (Nb1 at odd `it`, else Nb2) is read only for realisations with nzero = 0 and avok = 0; it is not required, so a
 * caller with such realisations supplies it (a NULL one holds the sentinel like any other buffer).
 *   state, state_out [batch][ACE_UNIT_NSTATE]: mu, last_res, opt_obj, nB, vbound, obj2, nAX2, nY2, nJM2, dY2, dAtY,
 *          nAtY, kf0, kf1, kf2, kf3, kfcum, pd_dZ2, pd_nZ2, pd_rc, fs0, fs3   (NULL state: zeros, mu = 1)
 *   flags, flags_out [batch][ACE_UNIT_NFLAG]: iters, done, status, nzero, avok, optsrc, optysrc, kfok, dpend, fzit,
 *          zit, mzit, msp, z0id, msp_pad, mres
 *   done_count / mspcount (and _out): the batch's counts of stopped realisations and of m-space steps before / after
 *   guard_ok: 1 when the control block after the batch's and every control-block field not listed above are as
 *          they were
 *   state_ext = 1: the rows of state and state_out have ACE_UNIT_NSTATE + 1 elements, the last one recert (the iteration
 *          of the realisation's last fresh-reference request, 0: none), and gyf_kernel may raise a request as in a
 *          solve with ACE_MSP_RECERT on; 0: the rows above, and no request is raised
 * Checked before any HIP call: ACE_ERR_ARG for an unknown op, batch, n or m < 1, a negative guard, it < 1, q not 0 / 1,
 * rho <= 0, np outside 0..4, it_end <= it or waves not 8 / 4 (MSR) and a NULL required array (named in
 * ace_last_error()); ACE_ERR_UNSUPPORTED for m > 256, for MSR at m != 256 and for a refused LDS request or a
 * codebook the int8 setup does not take.  Synchronous; allocates its own device memory. */
enum { ACE_UNIT_GYK = 0, ACE_UNIT_GYF, ACE_UNIT_AHF, ACE_UNIT_MSR, ACE_UNIT_READY, ACE_UNIT_OPTX, ACE_UNIT_NOPS };
#define ACE_UNIT_NSTATE 22
#define ACE_UNIT_NFLAG 16
typedef struct ace_unit_args {
    int32_t op, batch, n, m, it, it_end, maxiter, q, fixed_iters, guard, done_count, mspcount;
    int32_t lazy, use_la, use_ax, yn_copy, msp, ctl, np, msp_fail_it, waves, state_ext;
    double tol_rel, tol_abs, rho, room, sentinel;
    double fl[4];
    const double *A, *B, *T, *g, *Y0, *Y1, *KY0, *KY1, *M, *AX, *optY, *S0, *S1, *optS;
    const double *Zb1, *Zb2, *Nb1, *Nb2, *X, *Xcur, *optX, *state;
    const int32_t* flags;
    const unsigned char* rank_one;
    double *K_out, *G_out, *c_out;
    double *B_out, *T_out, *g_out, *Y0_out, *Y1_out, *KY0_out, *KY1_out, *M_out, *AX_out, *optY_out, *S0_out, *S1_out;
    double *optS_out, *Zb1_out, *Zb2_out, *Nb1_out, *Nb2_out, *X_out, *Xcur_out, *optX_out, *state_out;
    int32_t *flags_out, *done_count_out, *mspcount_out, *resume, *steps, *vecw, *ready, *guard_ok;
} ace_unit_args;
int ace_unit_host(const ace_unit_args* args);

/* ---- driver-level boundary (MATLAB Engine calls of main/main.py:308, :427-437) ------------
 *   [H_amp,H_angle] = channel_recovery_ADMM_v2_simulation_<A2only|A2nuclear|multiresolution|phaselift>(
 *                         tx_ant_num, rx_ant_num, cb_amp, cb_angle, rss_final, seed_id)
 *   main/channel_recovery_ADMM_v2_simulation_A2only.m:9-179 (A2nuclear, multiresolution, phaselift
 *   alike; phaselift runs MyPhaseLift per sweep point, Recover_Channel.m:32-35).
 * cb_amp / cb_angle: HOST [P][n] row-major f64 (codebook row p = beam p; MATLAB callers pass
 * the transpose of their P x n arrays), rss_dbm: [P] (dBm).  M_list = NULL selects the
 * reference sweep round(linspace(2, sqrt(4*tx*rx), 8)).^2 (:106-118).  Outputs H_amp, H_angle:
 * HOST [n_M][n] row-major (MATLAB's n_M x 1 x n squeezed), element k in vec(H) order
 * (i + tx*j).  Returns the number of sweep points (>= 1) or a negative error code.
 * Row selection uses the build's RNG seeded from the reference seed lists (MATLAB streams are
 * not reproducible outside MATLAB).  Sweep points with floor(0.95 M) < min(20, M) train rows
 * (M = 4) are ill-posed for the spectral initialisation and return 0 (the reference's
 * NaN -> 0 of :176). */
#define ACE_DRIVER_A2ONLY 0     /* channel_recovery_ADMM_v2_simulation_A2only.m */
#define ACE_DRIVER_A2NUCLEAR 1  /* channel_recovery_ADMM_v2_simulation_A2nuclear.m */
#define ACE_DRIVER_MULTIRES 2   /* channel_recovery_ADMM_v2_simulation_multiresolution.m.  The reference defines the
                                   tiers for 16 x 16 only (rows [1984, 3968, 3968], M <= 96 / <= 256 / else,
                                   ..._multiresolution.m:110-112,137-144); at 32 x 32 the build uses its own analogue
                                   (4x the rows: 7936/15872/15872, thresholds 384/1024) -- a builder-defined layout
                                   whose parity with any reference codebook is unpinned */
#define ACE_DRIVER_PHASELIFT 3  /* channel_recovery_ADMM_v2_simulation_phaselift.m (MyPhaseLift, rng(4096)) */
int ace_recover_driver(int driver, int tx, int rx, int P, const double* cb_amp, const double* cb_angle,
                       const double* rss_dbm, int seed_id, int n_M, const int32_t* M_list,
                       double* H_amp, double* H_angle);
/* The same with the iteration cap of every solve in the call: maxiter > 0 replaces the reference's 500 ADMM
 * iterations per pipeline stage (inferLowRankV4_multi.m:13) or 4000 TFOCS iterations (MyPhaseLift.m:82);
 * 0 keeps them.  For parity runs on the horizon where the reference algorithm is stable against its own
 * rounding (the A2nuclear refinement). */
int ace_recover_driver_ex(int driver, int tx, int rx, int P, const double* cb_amp, const double* cb_angle,
                          const double* rss_dbm, int seed_id, int n_M, const int32_t* M_list, int maxiter,
                          double* H_amp, double* H_angle);
/* The reference M sweep for (tx, rx) into M_out[8]; returns 8 or a negative error code
 * (..._A2only.m:106-118, error :117). */
int ace_driver_m_sweep(int tx, int rx, int32_t* M_out);
/* First k entries of a uniform random permutation of 0..P-1 (randperm(P,k) / randsample,
 * 0-based, sampled order) from the build's counter RNG (seed, stream).  Host only. */
int ace_driver_randperm(uint64_t seed, uint64_t stream, int P, int k, int32_t* out);

/* ---- downstream beamformer ----------------------------------------
 *   wr_out, wt_out = svd_beamformer(H)                       main/codebook_library.py:57-96
 *   wr_out, wt_out = svd_beamformer_compensation(H, offset)  main/codebook_library.py:98-138
 *   reached from codebook_generator (:192-213), H = reshape(H_est[i,:], [tx, rx]) (:197).
 * H: [batch][tx][rx] c128 row-major (DEVICE for _batch), 1 <= tx, rx <= 32 (main.py:454 calls
 * it square; any shape np.shape(H) gives is taken, with zgesdd's QR / LQ / direct paths).
 * offset: [batch][max(tx, rx)] radians (compensation * pi/2; entry k compensates element k of
 * both codes, i.e. numpy's broadcasting — tx != rx admits only a constant row there) or NULL
 * for svd_beamformer.  Outputs: wr_code [batch][rx] and wt_code [batch][tx] (2-bit phase codes
 * 0..3 = the characters of the reference's strings), beam_idx [batch][2] = (tx_idx, rx_idx) of
 * the argmax pair, rss [batch] = its 10*log10(|wt^T H wr|^2 * 1000), status [batch]
 * (ACE_ST_BF_*).  vh_r [batch][rx][rx] / vh_t [batch][tx][tx] (optional, may be NULL): c128 Vh
 * of svd(H) and svd(H^T) in numpy's (zgesdd's) phase and sign convention. */
#define ACE_ST_BF_NONFINITE 16u /* H has NaN/Inf: numpy raises LinAlgError; codes zeroed, beam_idx -1 */
#define ACE_ST_BF_NOCONV 32u    /* dbdsqr iteration budget exhausted (numpy would raise) */
#define ACE_ST_BF_DC 64u        /* min(tx, rx) > 25: zgesdd's divide and conquer, its merge's signs applied;
                                   a vector the merge deflates (rank-deficient H) may still differ */
int ace_svd_beamformer_batch(int batch, int tx, int rx, const double* H, const double* offset,
                             uint8_t* wr_code, uint8_t* wt_code, int32_t* beam_idx, double* rss,
                             uint32_t* status, double* vh_r, double* vh_t, void* stream);
int ace_svd_beamformer_host(int batch, int tx, int rx, const double* H, const double* offset,
                            uint8_t* wr_code, uint8_t* wt_code, int32_t* beam_idx, double* rss,
                            uint32_t* status, double* vh_r, double* vh_t);

/* ---- channel evaluation (the reference's parity metric) ----------------------
 * Evaluation_H (Numerical_Simulation/src/evaluate_plot_results/Evaluation_H.m:73-132), batched.
 * X, G: [batch][n] c128 DEVICE (n = tx*rx, vec(H) order); metrics: [batch][4] f64 DEVICE
 * = {nmse, gain_ana, gain_dig, proj_err}; status [batch] (may be NULL).  Asynchronous on stream.
 *   nmse     = ||g - ((x^H g)/(x^H x)) x||^2 / ||g||^2                         (:87-89)
 *   gain_ana = |Q(u1)^H mat(g) Q(v1)|, Q = Quantize_PS at 2 bits                (:95-99, :103)
 *   gain_dig = |u1^H mat(g) v1| with unit u1, v1                                (:100-104)
 *   proj_err = ||X_g - ((X^H X_g)/(X^H X)) X|| / ||X_g||, X / X_g the rank-one parts of
 *              mat(x) / mat(g)                                                  (:107-115)
 * u1, v1 are the top singular vectors of mat(x) (tx x rx, entry (i, j) = x[i + tx*j]) in the gauge
 * of ace_svd_beamformer_batch: v1 = conj(row 0 of vh_r), u1 = row 0 of vh_t.  gain_ana is invariant
 * under powers of j on u1 or v1, so the divide-and-conquer sign (ACE_ST_BF_DC) does not reach it;
 * the other metrics are gauge-free.  1 <= tx, rx <= 32, batch >= 1; bad shapes and NULL X, G or
 * metrics return ACE_ERR_ARG before any HIP call.
 * Departure from the reference: an x or g that is all zero or not finite (where the reference
 * returns NaN or an arbitrary basis vector) gives nmse = 1, proj_err = 1, both gains 0 and
 * ACE_ST_EVAL_DEGENERATE, so Monte-Carlo means stay finite and the flag can be counted.
 * ACE_ST_BF_NOCONV: an SVD exhausted its iteration budget. */
#define ACE_ST_EVAL_DEGENERATE 256u
int ace_evaluate_batch(int batch, int tx, int rx, const double* X, const double* G,
                       double* metrics, uint32_t* status, void* stream);
int ace_evaluate_host(int batch, int tx, int rx, const double* X, const double* G,
                      double* metrics, uint32_t* status);   /* allocates, copies, synchronous */

/* ---- held-out RSS evaluation (the testbed's accuracy metric) --------------------------------
 * Evaluate_rss.m (main/src/evaluate_plot_results/ and Numerical_Simulation/src/evaluate_plot_results/),
 * batched:  rss_eval = abs(cb_test * H),  Evaluation = mean(abs(rss_eval - rss_test) ./ rss_test).
 * X [batch][n] c128; CB [Pt][n] c128 row-major (row p = test beam p, shared by the batch); rss
 * [rss_shared ? 1 : batch][Pt] f64 measured AMPLITUDES in X's units (not dBm); all DEVICE.
 * metrics [batch][4] f64 = {mean_rel, rms_rel, max_rel, n_used}; pred [batch][Pt] f64 = |CB x_b|, may be
 * NULL; status [batch], may be NULL.  Asynchronous on stream; no allocation, no host synchronisation.
 *   rel_p    = | |sum_k CB[p][k] X[b][k]| - rss_p | / rss_p     (no conjugate on CB: the product is cb_test * H)
 *   mean_rel = mean of rel_p over the usable rows (the reference's Evaluation); rms_rel, max_rel their
 *              root mean square and maximum; n_used the number of usable rows.
 * n need not be tx*rx (the metric never reshapes).  A realisation's four numbers and its pred row are a
 * function of (X_b, CB, rss_b, n, Pt) alone: not of batch, of b, or of pred being requested.
 * batch, n or Pt < 1, a NULL X, CB, rss or metrics and an rss_shared other than 0 or 1 return ACE_ERR_ARG
 * before any HIP call.
 * Departures from the reference, which gives Inf or NaN in these cases:
 *   - a test row whose rss_p is not finite or is <= 0 is left out of the three statistics and of n_used,
 *     and ACE_ST_RSS_SKIPPED is set; pred is still written for that row;
 *   - a realisation whose X has a non-finite entry, or that has no usable row (or whose statistics
 *     overflow), returns 1, 1, 1 and n_used = 0 with ACE_ST_EVAL_DEGENERATE (its pred row is whatever the
 *     product gives);
 *   - an all-zero X is not degenerate: pred = 0 and rel_p = 1 on its own. */
#define ACE_ST_RSS_SKIPPED 512u
int ace_rss_evaluate_batch(int batch, int n, int Pt, const double* X, const double* CB, const double* rss,
                           int rss_shared, double* metrics, double* pred, uint32_t* status, void* stream);
int ace_rss_evaluate_host(int batch, int n, int Pt, const double* X, const double* CB, const double* rss,
                          int rss_shared, double* metrics, double* pred,
                          uint32_t* status);   /* allocates, copies, synchronous */

/* ---- beam scan (exhaustive sweep and angular map) ----------------------------------------------
 * MyBeamSweeping.m:93-125 (RSS = |kron(transpose(F), W') vec(H) + noise|^2 and its argmax) and the angular
 * map Leakage = A_Rx' * H * A_Tx of Sparse_Channel_Formulation.m:149, batched and fused with the selection.
 * X [batch][d0*d1] c128 with mat(x)(i, j) = x[i + d0*j] (the layout ace_evaluate_batch takes); W0 [Q0][d0]
 * c128 row-major, beams on the leading index, applied conjugated; F1 [Q1][d1] c128 row-major, beams on the
 * trailing index, applied plain; noise NULL or [batch][Q1*Q0] c128; all DEVICE.
 *   y[b][p][q] = sum_i sum_j conj(W0[q][i]) x_b[i + d0*j] F1[p][j]      (w' * H * f)
 *   P          = |y + noise|^2,   flat index f = p*Q0 + q                (:124-125 zero-based: p = ind_F - 1, q = ind_W - 1)
 * top_pow, top_idx [batch][K]: the K largest P of the realisation in descending order, equal powers by
 * increasing f; total [batch] (may be NULL): the sum of P; power [batch][Q1*Q0] (may be NULL): the whole
 * map; status [batch] (may be NULL).  Asynchronous on stream; no allocation, no host synchronisation, no
 * workspace.  A realisation's outputs are a function of (x_b, W0, F1, noise_b, the sizes, K) alone: not of
 * batch, of b, of power or total being requested, or of the stream.
 * 1 <= d0, d1 <= 32, 1 <= Q0, Q1 <= 4096, 1 <= K <= min(16, Q0*Q1), batch >= 1; bad sizes and a NULL X, W0,
 * F1, top_pow or top_idx return ACE_ERR_ARG before any HIP call.  ACE_ERR_UNSUPPORTED when the kernel's
 * dynamic LDS request is refused.
 * A realisation whose x, or whose noise row, holds a non-finite value returns powers 0, indices -1, total 0
 * and ACE_ST_EVAL_DEGENERATE (its power row is whatever the product gives); an all-zero x is not degenerate.
 * A non-finite beam entry is the caller's error and is not checked. */
int ace_beam_scan_batch(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0,
                        const double* F1, const double* noise, int K, double* top_pow, int32_t* top_idx,
                        double* total, double* power, uint32_t* status, void* stream);
int ace_beam_scan_host(int batch, int d0, int d1, int Q0, int Q1, const double* X, const double* W0,
                       const double* F1, const double* noise, int K, double* top_pow, int32_t* top_idx,
                       double* total, double* power, uint32_t* status);   /* allocates, copies, synchronous */

/* ---- sparse-recovery evaluation (Evaluation_Recovery) ------------------------------------------------
 * Numerical_Simulation/src/evaluate_plot_results/Evaluation_Recovery.m:73-338, batched against one shared pair of
 * cut steering dictionaries: the score the reference gives PLOMP, PLGAMP, PerfectPhaseCS, NoisyPhaseCS and PRGAMP.
 * Per call: A_t [Qt][tx], A_r [Qr][rx] c128 (the rows of the cut dictionaries; AD = kron(conj(A_t), A_r), column
 * u Qr + v); deg_t [Qt], deg_r [Qr] f64, the grid angles in degrees (:105-113: rad2deg(asin(virtual / kappa)));
 * first_t, first_r: the global grid index of the first cut column per side, so that column 0 is in the reference's
 * index units; noise_power > 0; kappa = 2 pi d / lambda > 0.
 * Per realisation: z [batch][Qt*Qr] c128; vecH [batch][tx*rx] c128 (element r + rx t); aod_deg, aoa_deg [batch][L]
 * f64, the true angles; true_idx [batch][L][2] int32, the true paths' nearest global grid indices (AoD, AoA:
 * Quan_Pos_Err_h_array(2, l, 1:2) of Sparse_Channel_Formulation.m:98-103; only path 0 is read, for L == 1);
 * picks NULL or [batch][2][2] int32: (ind_F, ind_W) zero-based of pattern 1 and of pattern 2, as ace_beam_scan_batch
 * picks them, with the tables centre_deg_t [Mt], centre_deg_r [Mr] (pattern 2's estimate and both patterns' beams:
 * the 2-bit quantised steering vectors at the centres) and peak_deg_t [Mt], peak_deg_r [Mr] (pattern 1's estimate,
 * ace_beam_peak_angles).  The sweep is not redone.  All DEVICE.
 * metrics [batch][15] f64, the order of :322-336: Num_Quantization_Error, AoDA_Err, MSE_ARM, MSE_H,
 * Rate_Unconstrained, Rate_PerCSI, Rate_Est, Rate_Est_AoDA, Rate_BSweep1, Rate_BSweep2, AoDA_Err_Sweep1,
 * AoDA_Err_Sweep2, gain_ana, gain_dig, proj_error.  H_est [batch][tx*rx] c128 (may be NULL): AD z after the global
 * phase of :188-189, the reference's second output.  status [batch] (may be NULL).
 * The reference's behaviour as it stands (the L picks by modulus in ascending index order; the true AoD sorted
 * descending while :128 leaves the true AoA unsorted; the quantisation error for L == 1 only; Num_RFchains = 1, so
 * every beam is Quantize_PS'd at 2 bits; the AoDA beams at the LAST sorted estimate; det(eye(L) + scalar) =
 * 1 + L |g|^2 / noise_power; columns 12-14 = Evaluation_H of (H_est, H), in ace_evaluate_batch(H_est, H, rx, tx)'s
 * gauge) is listed in csrc/ace_receval.hip.  An exact modulus tie goes to the lower index (MATLAB: by phase angle).
 * H_est is formed as A_r^T mat(z)^T conj(A_t) on the f64 matrix cores; z is read once.  One wavefront per realisation;
 * a realisation's outputs are a function of its own inputs and the per-call tables alone.  Asynchronous on stream,
 * no allocation, nothing read back, no workspace.
 * Limits: 1 <= tx, rx <= 32, 1 <= L <= 8, 1 <= Qt, Qr <= 4096, 1 <= Mt, Mr <= 4096 (ACE_ERR_UNSUPPORTED above,
 * ACE_ERR_ARG below); batch < 1, L > Qt Qr, a negative first index, a noise_power or kappa that is not positive and
 * finite, a NULL required array (named in ace_last_error()) and picks without all four tables return ACE_ERR_ARG;
 * all of it before any HIP call.  ACE_ERR_UNSUPPORTED when the kernel's dynamic LDS request is refused.
 * Degenerate realisations (z or H not finite or all zero, an H_est that is zero or not finite, a metric that
 * overflows): MSE_H = MSE_ARM = proj_error = 1, gains and rates 0, H_est zeros, ACE_ST_EVAL_DEGENERATE; with a
 * degenerate z the angle columns are those of the picks 0 .. L - 1.  Without picks, or for a row with a pick outside
 * its table (the scan's -1), columns 8-11 are NaN and ACE_ST_RECEVAL_NOSWEEP is set.  ACE_ST_BF_NOCONV as above. */
#define ACE_ST_RECEVAL_NOSWEEP 131072u
#define ACE_RECEVAL_NCOL 15
int ace_evaluate_recovery_batch(int batch, int tx, int rx, int L, int Qt, int Qr, const double* A_t,
                                const double* A_r, const double* deg_t, const double* deg_r, int first_t,
                                int first_r, double noise_power, double kappa, const double* z, const double* vecH,
                                const double* aod_deg, const double* aoa_deg, const int32_t* true_idx,
                                const int32_t* picks, int Mt, int Mr, const double* centre_deg_t,
                                const double* centre_deg_r, const double* peak_deg_t, const double* peak_deg_r,
                                double* metrics, double* H_est, uint32_t* status, void* stream);
int ace_evaluate_recovery_host(int batch, int tx, int rx, int L, int Qt, int Qr, const double* A_t,
                               const double* A_r, const double* deg_t, const double* deg_r, int first_t,
                               int first_r, double noise_power, double kappa, const double* z, const double* vecH,
                               const double* aod_deg, const double* aoa_deg, const int32_t* true_idx,
                               const int32_t* picks, int Mt, int Mr, const double* centre_deg_t,
                               const double* centre_deg_r, const double* peak_deg_t, const double* peak_deg_r,
                               double* metrics, double* H_est, uint32_t* status);   /* allocates, copies, synchronous */

/* Pattern 1's angle estimate of the sweep (MyBeamSweeping.m:134-154): for each of M beams [M][N] c128 (DEVICE), the
 * first angle of -90 : 0.005 : 90 degrees (36001 points, built from both ends as MATLAB's colon does) that maximises
 * |f^H a(theta)|, a(theta)[k] = exp(-j kappa sin(theta) k).  peak_deg [M] f64 (DEVICE); NaN for a beam with a
 * non-finite entry.  Once per sweep point, not per realisation.  1 <= N <= 32 (ACE_ERR_UNSUPPORTED above), M >= 1;
 * asynchronous on stream. */
int ace_beam_peak_angles(int M, int N, double kappa, const double* beams, double* peak_deg, void* stream);
int ace_beam_peak_angles_host(int M, int N, double kappa, const double* beams, double* peak_deg);   /* allocates, copies, synchronous */

/* ---- batched orthogonal matching pursuit (the sparse stage of PLOMP and of the coherent CS benchmark) ----
 * The reference calls OMP(C, intSoln, 1e-12) (My_TwoStage_Recovery.m) and OMP(A, y, s) (My_Conventional_CS.m);
 * OMP.m itself belongs to the external CoSaMP_OMP toolbox and is not in the reference tree.  This is textbook
 * OMP with both stopping rules; "a third argument below 1 is a tolerance" is this project's reading of the call
 * sites, not a transcription.  Per realisation, against one shared dictionary:
 *   r = y, I = {};  repeat: stop if |I| = kmax or ||r||_2 <= tol;
 *                           j = argmax over j not in I of w_j |d_j^H r|^2   (ties: smaller j; w = colscale or 1);
 *                           I <- I u {j};  c = argmin ||y - D_I c||_2;  r = y - D_I c
 * D [d][N] c128 row-major (column j = atom j, shared by the batch); colscale NULL or [N] f64; Y [batch][d]
 * c128; all DEVICE.  Outputs: idx [batch][kmax] int32 in selection order, -1 past count; coef [batch][kmax]
 * c128 in the same order, 0 past count; count [batch] int32; resnorm [batch] f64, the final ||r||_2; status
 * [batch] (may be NULL); x [batch][N] c128 (may be NULL), the dense solution.  workspace: at least
 * ace_omp_workspace_size(batch, d, N, kmax) bytes of DEVICE memory (the progressive QR factors of D_I, built by
 * modified Gram-Schmidt); ACE_ERR_WORKSPACE when NULL or shorter.  Asynchronous on stream; no allocation, no
 * host synchronisation, no atomics.  A realisation's outputs are a function of (y_b, D, colscale, d, N, kmax,
 * tol) alone: not of batch, of b, of x being requested, or of the stream.
 * Limits: 1 <= d <= 256, 1 <= N <= 16384, 1 <= kmax <= min(d, N), tol >= 0, batch >= 1.  A size below 1, a
 * kmax beyond min(d, N), a tol that is negative or NaN and a NULL D, Y, idx, coef, count or resnorm return
 * ACE_ERR_ARG; d > 256 or N > 16384, or a refused dynamic LDS request, return ACE_ERR_UNSUPPORTED; all of it
 * before any HIP call.  There is no second path and no CPU fallback.  ace_omp_workspace_size returns 0 for
 * sizes outside the limits.
 * Departures from a textbook OMP / the reference's call:
 *   - a non-finite entry of y_b gives count 0, indices -1, resnorm 0 and ACE_ST_EVAL_DEGENERATE;
 *   - y_b = 0, or ||y_b|| <= tol, gives count 0 and no flag;
 *   - a selected atom whose part orthogonal to the span of the chosen atoms has norm <= 2^-26 ||d_j|| (sqrt(u):
 *     with it kappa_2(D_I) >= 2^26 and the coefficients would keep fewer than half their digits) is NOT added;
 *     the realisation stops there and sets ACE_ST_OMP_DEPENDENT.  An all-zero atom is dependent by that test.
 * A non-finite entry of D or colscale is the caller's error and is not checked. */
#define ACE_ST_OMP_DEPENDENT 1024u
size_t ace_omp_workspace_size(int batch, int d, int N, int kmax);
int ace_omp_solve_batch(int batch, int d, int N, int kmax, double tol, const double* D, const double* colscale,
                        const double* Y, int32_t* idx, double* coef, int32_t* count, double* resnorm,
                        uint32_t* status, double* x, void* workspace, size_t workspace_bytes, void* stream);
int ace_omp_solve_host(int batch, int d, int N, int kmax, double tol, const double* D, const double* colscale,
                       const double* Y, int32_t* idx, double* coef, int32_t* count, double* resnorm,
                       uint32_t* status, double* x);   /* host arrays; allocates, copies, synchronous */

/* ---- batched EM-BG-GAMP (the sparse stage of PLGAMP and the first branch of My_Conventional_CS.m) ----------
 * EMBGAMP(y, D, optEM) of the reference's vendored GAMP package (3rd_software_component/GAMP/trunk/code:
 * EMGMAMP/EMBGAMP.m -> EMGMAMP/EMGMAMP.m, main/gampEst.m, CAwgnEstimIn, CAwgnEstimOut, SparseScaEstim,
 * EMGMAMP/CBG_update.m, set_initsBG.m; MATLAB's genpath puts EMGMAMP/ ahead of EMGMAMPnew/), restated for a batch
 * of independent realisations (T = 1 column each) against one shared dictionary: expectation-maximisation over a
 * Bernoulli-Gaussian prior (lambda, phi; theta = 0) and the noise variance psi around generalised approximate
 * message passing with adaptive damping.  One launch runs every EM iteration, every GAMP iteration and the final
 * GAMP call (csrc/ace_gamp.hip states the iteration and the reference's quirks it keeps).
 * cfg: the two option sets the reference uses differ in learn_lambda only --
 *   PLGAMP (My_TwoStage_Recovery.m:165-172): learn_lambda 0;  My_Conventional_CS.m:71-77: learn_lambda 1;
 *   both: SNRdB given (capped at 100), lambda0 = s / n, maxEMiter 200, robust_gamp (nit 25, step 0.1), tol 1e-5.
 * max_em_iter = 0 skips the EM loop: one GAMP call from a cold start (the kernel-level tests' handle).
 * D [d][N] c128 row-major, Y [batch][d] c128, DEVICE.  Outputs: xhat [batch][N] c128; xvar [batch][N] f64 (may be
 * NULL); params [batch][3] f64 = lambda, phi, psi at exit; em_iters [batch] int32, the EM iterations started; trace
 * (may be NULL) [batch][max_em_iter + 1][2] int32, per gampEst call its iterations and the bit mask of its passed
 * iterations (bit it - 1), the final call in slot em_iters, unused slots 0; status [batch] (may be NULL).
 * workspace: ace_gamp_workspace_size(batch, d, N) bytes of DEVICE memory (the N-long and d-long state vectors:
 * 144 B per atom and 112 B per row, per realisation rounded up to 16); ACE_ERR_WORKSPACE when NULL or shorter.
 * Asynchronous on stream; no allocation, no host synchronisation, no atomics.  A realisation's outputs are a
 * function of (y_b, D, cfg, d, N) alone.
 * Limits: 1 <= d <= 256, 1 <= N <= 16384, batch >= 1, 0 < lambda0 <= 1, max_em_iter >= 0, 1 <= gamp_nit <= 31,
 * 0 < step0 <= 1, gamp_tol >= 0, snr_db finite; a NULL cfg, D, Y, xhat, params or em_iters and a value outside
 * these return ACE_ERR_ARG, d > 256 or N > 16384 or a refused dynamic LDS request ACE_ERR_UNSUPPORTED, all before
 * any HIP call.  ace_gamp_workspace_size returns 0 for sizes outside the limits.
 * Status:
 *   ACE_ST_GAMP_NANBREAK  the EM loop left through EMGMAMP.m:320 (a GAMP call with a single passed iteration leaves
 *                         rhat NaN); the final call still ran, from the entry state of the call that broke
 *                         (EMGMAMP.m breaks before that call's warm start is taken);
 *   ACE_ST_GAMP_MAXEM     the EM loop left at max_em_iter without meeting its tolerance;
 *   ACE_ST_GAMP_FAILED    the reference would raise, and its callers' catch falls back to OMP: xhat is zeroed.
 *                         Reachable with these options: CAwgnEstimOut's assert(wvar >= 0) (psi NaN or negative);
 *                         CAwgnEstimIn's assert(var0 > 0) on the initial phi (y = 0, or ||y||^2 overflowing); the NaN
 *                         break in the first EM iteration (the post-loop update reads an unassigned Shat);
 *   ACE_ST_EVAL_DEGENERATE  a non-finite entry of y_b: zeros, em_iters 0. */
#define ACE_ST_GAMP_NANBREAK 2048u
#define ACE_ST_GAMP_MAXEM 4096u
#define ACE_ST_GAMP_FAILED 8192u
typedef struct ace_gamp_cfg {
    double snr_db;      /* optEM.SNRdB: initialises psi = ||y||^2 / (d (1 + 10^(min(100, SNRdB) / 10))) */
    double lambda0;     /* optEM.lambda: the sparsity rate, s / n in both call sites */
    int learn_lambda;   /* optEM.learn_lambda */
    int max_em_iter;    /* optEM.maxEMiter (200); 0: no EM loop, one cold GAMP call */
    int gamp_nit;       /* optGAMP.nit (25 with robust_gamp) */
    int reserved;
    double step0;       /* optGAMP.step (0.1 with robust_gamp) */
    double gamp_tol;    /* optGAMP.tol (1e-5) */
} ace_gamp_cfg;
void ace_gamp_cfg_default(ace_gamp_cfg* cfg);   /* the PLGAMP set; snr_db 0, lambda0 0 (the caller's to set) */
size_t ace_gamp_workspace_size(int batch, int d, int N);
int ace_gamp_solve_batch(const ace_gamp_cfg* cfg, int batch, int d, int N, const double* D, const double* Y,
                         double* xhat, double* xvar, double* params, int32_t* em_iters, int32_t* trace,
                         uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int ace_gamp_solve_host(const ace_gamp_cfg* cfg, int batch, int d, int N, const double* D, const double* Y,
                        double* xhat, double* xvar, double* params, int32_t* em_iters, int32_t* trace,
                        uint32_t* status);   /* host arrays; allocates, copies, synchronous */

/* ---- batched PR-GAMP (Method.PRGAMP of Vs_M.m: MyCPR.m:110-120 -> MyPRGAMP.m:71 -> prGAMP4) --------------
 * prGAMP4(abs_y, D, opt_pr) of the reference's vendored GAMP package (3rd_software_component/GAMP/trunk/code:
 * phase/prGAMP4.m, phase/ncCAwgnEstimOut.m, main/gampEst.m, main/estimInvert.m, main/CAwgnEstimIn.m,
 * main/SparseScaEstim.m, main/GampOpt.m), restated for a batch of independent realisations (T = 1 column each)
 * against one shared matrix: compressive phase retrieval straight from the magnitudes |D x + w|, without the PhaseLift
 * compression stage.  Generalised approximate message passing under the non-coherent output channel (a Bessel ratio in
 * the posterior, the Bethe cost with its fixed-point inversion for the adaptive step, variance normalisation, a damped
 * pvar, a window of passed utilities), inside an EM loop that learns the noise variance and tunes the
 * Bernoulli-Gaussian prior, inside random restarts.  One launch runs every try, every EM iteration and every GAMP
 * iteration (csrc/ace_prgamp.hip states the iteration, the fixed options and the reference's quirks it keeps).
 * cfg: the MyCPR.m set is ace_prgamp_cfg_default with sparse_rat = s / n.  gamp_nit, nit_em and max_try may be set
 * small (8, 0, 1: one short cold GAMP call, the kernel-level tests' handle).
 * D [m][N] c128 row-major, Y [batch][m] f64 (the magnitudes; MyPRGAMP passes sqrt of the squared measurements; the
 * absolute value is taken), G [batch][max_try][N] c128: the restart draws, standing for randn(nx, 2) * [1; 1i] of
 * prGAMP4.m:608 (real and imaginary parts of unit variance; MATLAB's stream cannot be reproduced, so they are the
 * caller's) -- 16 batch max_try N bytes, 26.8 GB at batch 4096, N 4096 and the reference's 100 tries: a caller
 * sweeping many realisations at the full try count goes in chunks.  All DEVICE.
 * Outputs: xhat [batch][N] c128, the best try's estimate; info [batch][8] f64 = the best residual
 * 20 log10(|| |D xhat| - y || / ||y||) in dB, the noise variance wvar_hat of the best try's last EM iteration,
 * sparseRat_hat, xvar0_hat (both of the LAST try, as out.sparseRat_hat / out.xvar0_hat are), xmean0sq_hat (0: the
 * mean is not tuned), SNRdB_est of the best try's last EM iteration, two reserved zeros; counts [batch][4] int32 =
 * numTry, the best try (1-based), the EM iterations of the best try, support_size (-1 where the reference leaves it
 * NaN: no try reached the stop level); status [batch] (may be NULL); trace (may be NULL) [batch][max_try][nit_em + 1][2]
 * int32, per gampEst call its iterations and its passed iterations, 0 for calls that did not run; vals (may be NULL)
 * [batch][max_try][nit_em + 1] f64, the last passed utility of each call.
 * workspace: ace_prgamp_workspace_size(batch, m, N, max_try) bytes of DEVICE memory (the N-long and m-long state
 * vectors: 184 B per atom and 192 B per row, per realisation rounded up to 16); ACE_ERR_WORKSPACE when NULL or
 * shorter.  Asynchronous on stream; no allocation, no host synchronisation, no atomics.  A realisation's outputs are a
 * function of (y_b, G_b, D, cfg, m, N) alone.
 * Limits: 1 <= m <= 256, 1 <= N <= 16384, batch >= 1, 0 < sparse_rat <= 1, snr_db and snr_db_init finite (capped at
 * 100), max_try >= 1, nit_em >= 0, gamp_nit >= 1; a NULL cfg, D, Y, G, xhat, info or counts and a value outside these
 * return ACE_ERR_ARG, m > 256 or N > 16384 or a refused dynamic LDS request ACE_ERR_UNSUPPORTED, all before any HIP
 * call.  ace_prgamp_workspace_size returns 0 for sizes outside the limits.
 * Status:
 *   ACE_ST_PRGAMP_FAILED  the reference would raise and MyPRGAMP's catch returns zeros: xhat and info are zeroed.
 *                         Reachable: CAwgnEstimIn's assert(var0 > 0) on xvar0 (y = 0) or on a tuned var0 that is NaN
 *                         or <= 0; estFin_best never assigned because every try ended with a NaN or Inf residual
 *                         (a y whose squared norm overflows ends there and is failed at once);
 *   ACE_ST_PRGAMP_MAXTRY  the tries ran out above the stop level -(snr_db + 2) dB: xhat is the best try, as in the
 *                         reference;
 *   ACE_ST_EVAL_DEGENERATE  a non-finite entry of y_b: zeros. */
#define ACE_ST_PRGAMP_FAILED 16384u
#define ACE_ST_PRGAMP_MAXTRY 32768u
typedef struct ace_prgamp_cfg {
    double sparse_rat;    /* opt_pr.sparseRat: s / n (the kernel applies tuneOn's min(., 0.9)) */
    double snr_db_init;   /* opt_pr.SNRdBinit (20): the first noise variance mean(y^2) / (1 + 10^(./10)) */
    double snr_db;        /* opt_pr.SNRdB (25): xvar0 and the stop level -(SNRdB + 2) dB */
    int max_try;          /* opt_pr.maxTry (100) */
    int nit_em;           /* opt_pr.nitEM (50): up to nit_em + 1 gampEst calls per try */
    int gamp_nit;         /* opt_gamp_init.nit (200) */
    int reserved;
} ace_prgamp_cfg;
void ace_prgamp_cfg_default(ace_prgamp_cfg* cfg);   /* the MyCPR.m set; sparse_rat 0 (the caller's to set) */
size_t ace_prgamp_workspace_size(int batch, int m, int N, int max_try);
int ace_prgamp_solve_batch(const ace_prgamp_cfg* cfg, int batch, int m, int N, const double* D, const double* Y,
                           const double* G, double* xhat, double* info, int32_t* counts, uint32_t* status,
                           int32_t* trace, double* vals, void* workspace, size_t workspace_bytes, void* stream);
int ace_prgamp_solve_host(const ace_prgamp_cfg* cfg, int batch, int m, int N, const double* D, const double* Y,
                          const double* G, double* xhat, double* info, int32_t* counts, uint32_t* status,
                          int32_t* trace, double* vals);   /* host arrays; allocates, copies, synchronous */

/* ---- batched min-L2 ADMM (Method.ADMM of Vs_M.m: ADMM_v2(..., version 0) -> inferMinL2.m) ------------------
 * InferADMM of ADMM_v2/inferMinL2.m:229-326 with lambda = 0 (the only value a caller passes), restated for a batch
 * of realisations against one shared A: the 2ACE iteration without the low-rank Z-block,
 *   X = pinv(A) (Y - M / mu),  Y = ArgMinY(A X, B, M, mu),  M += mu (A X - Y),
 * with the best-objective iterate, the residuals and thresholds of :304-310 (sqrt(m r), sqrt(n r), sqrt(2 m r)), the
 * stop test and mu *= rho while the combined residual is above 0.9 of the last one.  One launch runs the
 * initialisation (:244-257) and every iteration of one call for the whole batch (csrc/ace_minl2.hip); the three
 * m x n products of an iteration run on the f64 matrix cores.
 * ace_minl2_admm_batch: one InferADMM call.  A [m][n] c128 row-major, B [batch][m] f64, X0 [batch][r][n] c128
 * (column j of realisation b at X0[b][j][:]), rcols [batch] int32 or NULL: the columns of realisation b that exist
 * (clipped to 1 .. r; NULL: r for all) -- columns at and beyond rcols[b] are never read and never influence a result;
 * scale_by_row 1: the row form (the r columns share the row norm; X [batch][r][n] and Y [batch][r][m] return all
 * columns, zeros beyond rcols[b]), 0: the per-column form (X [batch][n], Y [batch][m]: the column with the smallest
 * objective, first index, NaN skipped as MATLAB's min does).  All DEVICE.  Further outputs, each may be NULL: Xall
 * [batch][r][n], every column of the iterate at the best iteration; iters [batch] int32, the iterations run; objcol
 * [batch] int32, the column returned (0 in the row form); opt_obj [batch] f64, the best objective || |A X| - B ||; mu
 * [batch] f64 at exit; status [batch]: ACE_ST_CONVERGED when the stop test passed, ACE_ST_NO_OPT when no objective was
 * ever finite (the last iterate is returned; the reference would raise).
 * workspace: ace_minl2_workspace_size(batch, m, n, r) bytes of DEVICE memory (pinv(A), the Gram matrix and its
 * Cholesky factor, and 16 (5 m + 4 n) 32 B of state per work-group: one per realisation with r > 1, one per 32
 * realisations with r = 1); ACE_ERR_WORKSPACE when NULL or shorter.  Synchronises the stream once (the pivot test of
 * the setup), then asynchronous; no allocation, no atomics.  A realisation's outputs are a function of its own B, X0
 * and rcols entry, A, the sizes and cfg alone.
 * cfg: r, cc_frac and train_seed belong to the whole recovery (inferMinL2); a stage reads maxiter, mu0, rho, tol_rel
 * and tol_abs.
 * Limits: 1 <= n <= 1024, 1 <= m <= 4096, 1 <= r <= 32, batch >= 1, maxiter >= 1, mu0 and rho positive, tolerances
 * not negative; a NULL cfg, A, B, X0, X or Y and a value outside these return ACE_ERR_ARG before any HIP call.
 * ace_minl2_workspace_size returns 0 for sizes outside the limits.
 * Departures from the reference:
 *   - pinv(A) is formed through the Cholesky factor of A^H A (m > n) or A A^H; a pivot at rounding level of its
 *     diagonal entry (rank-deficient A) returns ACE_ERR_UNSUPPORTED where MATLAB's pinv would truncate the singular
 *     value -- the contract ace_phaselift_solve_batch has for m <= n;
 *   - m <= n: A pinv(A) = I is used exactly (A X is Y - M / mu itself, not the rounded product), so the stage stops
 *     after one iteration with an objective at rounding level, as the reference does up to its rounding;
 *   - m <= n, per-column form: every column's objective is at rounding level, so which column is "best" is decided by
 *     rounding noise, here as in the reference (two float64 runs of the reference differ in it).
 *
 * ace_minl2_solve_batch: the whole of inferMinL2.  A /= ||A||_F / sqrt(m), B /= ||B|| (the tol_abs guards);
 * r = min(cfg->r, m, n); m_t = ceil(m cc_frac) train rows (ceil: inferLowRankV4 takes floor); on the train rows the
 * spectral initialisation, the column count of :187-190 per realisation (r_b = max(first k with 90 % of the
 * spectrum's sum, 3) where the r leading eigenvalues hold 90 %, then min(r_b, m_t, n): with r < 3 that can be MORE
 * than r, and min(max(r, 3), m_t, n) columns are initialised for it; the copy of that block at :203-206 changes
 * nothing), the row-form stage, X <- X eig(X^H X) (ascending, not re-sorted) and the per-column
 * stage; the quality 1 - || |A_te x| - B_te || / ||B_te|| on the test rows; where it exceeds 0.6 a row-form r = 1
 * stage on the full A from that x, rolled back at similarity < 0.6 (ACE_ST_ROLLBACK); X and Y scaled by
 * ||B|| / ||A||.  Without test rows (m < 20) the quality is NaN and there is no refinement, as in the reference.
 * train_idx: HOST array [m_t] of 0-based rows, ONE partition for the batch (the test rows are the sorted complement);
 * NULL draws it from the build's counter RNG (ace_driver_randperm(train_seed, 0, m, m_t)).
 * Outputs (DEVICE): X [batch][n], Y [batch][m] c128 (without refinement, or after a rollback, Y lives on the train
 * rows: its first m_t entries in train order, zeros beyond); may be NULL: quality [batch] f64, stage_iters [batch][3]
 * int32 (row stage, per-column stage, refinement; 0 where not run), r_used [batch] int32, status [batch]:
 * ACE_ST_CONVERGED (the stop test of the last stage the realisation ran), ACE_ST_NO_OPT (any stage),
 * ACE_ST_ROLLBACK, ACE_ST_EIG_NOCONV (the spectral initialisation or the rotation).
 * workspace: ace_minl2_solve_workspace_size(cfg, batch, m, n) bytes of DEVICE memory (0 outside the limits).
 * Realisations are solved in groups of equal column count, and the refinement on those that take it; a
 * realisation's outputs do not depend on the grouping.  NOT asynchronous: the host decides the groups and the
 * refinement set, so the call synchronises the stream at every host round trip -- the upload of the row table, the
 * read-back of the column counts, the upload of the groups' indices, the pivot test of each of the two pinv setups, the
 * read-back of the qualities and the upload of the refinement set (each upload waits before and after its copy) -- and
 * only the last launches (the refinement stage, the rollback and the rescaling) are still in flight when it returns.
 * Further departures:
 *   - per-realisation partitions are not supported: the per-realisation machinery of ace_pipeline_solve_batch is
 *     built around (I + K)^-1 and does not carry over.  Each realisation's marginal distribution is unchanged (the
 *     channels are independent of the partition);
 *   - a rank-deficient A_t, or A where a refinement runs, returns ACE_ERR_UNSUPPORTED;
 *   - the spectrum's sum is taken as the trace (the sum of B_i^2 over the nonzero rows of A_t) and the leading
 *     eigenvalues as the squared norms of the initialisation's columns. */
typedef struct ace_minl2_cfg {
    int r;             /* 20 (inferMinL2.m:3): the column count of the whole recovery before its 0.9-energy rule */
    int maxiter;       /* 500, every stage */
    int train_seed;    /* seed of the partition draw of the whole recovery */
    int reserved;
    double mu0;        /* 1e-3 (:260) */
    double rho;        /* 1.03 (:261) */
    double cc_frac;    /* 0.95 (:34; m_t = ceil(m cc_frac)) */
    double tol_rel;    /* 1e-4 */
    double tol_abs;    /* 1e-8 */
} ace_minl2_cfg;
void ace_minl2_cfg_default(ace_minl2_cfg* cfg);
size_t ace_minl2_workspace_size(int batch, int m, int n, int r);
int ace_minl2_admm_batch(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int scale_by_row, const double* A,
                         const double* B, const double* X0, const int32_t* rcols, double* X, double* Y, double* Xall,
                         int32_t* iters, int32_t* objcol, double* opt_obj, double* mu, uint32_t* status,
                         void* workspace, size_t workspace_bytes, void* stream);
int ace_minl2_admm_host(const ace_minl2_cfg* cfg, int batch, int m, int n, int r, int scale_by_row, const double* A,
                        const double* B, const double* X0, const int32_t* rcols, double* X, double* Y, double* Xall,
                        int32_t* iters, int32_t* objcol, double* opt_obj, double* mu,
                        uint32_t* status);   /* host arrays; allocates, copies, synchronous */
size_t ace_minl2_solve_workspace_size(const ace_minl2_cfg* cfg, int batch, int m, int n);
int ace_minl2_solve_batch(const ace_minl2_cfg* cfg, int batch, int m, int n, const double* A, const double* B,
                          const int32_t* train_idx_host, double* X, double* Y, double* quality, int32_t* stage_iters,
                          int32_t* r_used, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int ace_minl2_solve_host(const ace_minl2_cfg* cfg, int batch, int m, int n, const double* A, const double* B,
                         const int32_t* train_idx, double* X, double* Y, double* quality, int32_t* stage_iters,
                         int32_t* r_used, uint32_t* status);   /* host arrays; allocates, copies, synchronous */

/* ---- batched Bayesian A-optimal probe selection (Bayes_Beam.m:12 -> bayesAopt_complex.m:105-254) -------------
 * A Fedorov row exchange: pick nrows rows of the candidate codebook F [P][n] (c128, row-major, shared by the designs
 * of a call) that minimise trace((X^H X + kdiag I)^-1), the posterior variance of the channel estimate, with A = I
 * and no fixed rows as Bayes_Beam.m calls it.  Passes over the rows repeat while some row switched and
 * iter < maxiter; a row switches to the candidate of the smallest exchange value a when a < acutoff or the row is
 * still unassigned; ties go to the smaller candidate index (MATLAB's min), and duplicated candidate rows compare
 * equal.  csrc/ace_aopt.hip states the step and the kernels (the candidate sweeps run on the f64 matrix cores).
 * Design d has nrows[d] rows (1 .. nrows_max) and starts from the candidates init[d][0 .. nrows[d]) (an input, as
 * train_idx is elsewhere: MATLAB's unidrnd stream cannot be reproduced; the entries may repeat).
 * Outputs, DEVICE arrays: rowlist [designs][nrows_max] int32 (the candidate of every design row, -1 past nrows[d]),
 * acrit [designs][2] f64 (trace of the start's inverse, tracked value at the end), iters and switches [designs] int32
 * (passes run, rows switched), status [designs] uint32 (may be NULL), Minv_out NULL or [designs][n][n] c128 (the
 * tracked inverse of the final design).
 *   ACE_ST_AOPT_SINGULAR  1 - Re(x^H Minv x) of a row to remove was not positive and finite (or no exchange value
 *                         was): the design stopped there with its rows as they stand; the other designs go on.
 * A design's outputs are a function of (F, its nrows, its init, cfg) alone: not of the batch, of its place in it or
 * of Minv_out.  workspace: ace_aopt_workspace_size(designs, P, n, nrows_max) bytes of DEVICE memory (the inverses
 * and the start's scratch dominate: 16 n (n + min(nrows_max, n)) B per design); ACE_ERR_WORKSPACE when NULL or shorter.  The call enqueues on stream and
 * synchronises it once per pass (the test whether any design goes on); no allocation.
 * Limits: 1 <= n <= 1024, 1 <= P <= 65536, 1 <= nrows_max <= 4096 (ACE_ERR_UNSUPPORTED above, ACE_ERR_ARG below);
 * designs < 1, maxiter < 1, a kdiag that is not positive and finite, a non-finite acutoff and a NULL cfg, F, nrows,
 * init, rowlist, acrit, iters or switches return ACE_ERR_ARG; all of it before any HIP call.
 * ace_aopt_workspace_size returns 0 for sizes outside the limits.  nrows and init of ace_aopt_select_batch are device
 * arrays and cannot be checked there: the kernels clamp them into 1 .. nrows_max and 0 .. P - 1, so nothing is read
 * out of bounds.  ace_aopt_select_host checks them (ACE_ERR_ARG). */
#define ACE_ST_AOPT_SINGULAR 65536u
typedef struct ace_aopt_cfg {
    int maxiter;      /* passes over the rows, >= 1 (reference: 5) */
    int reserved;
    double kdiag;     /* kappa of K = kappa I (Bayes_Beam.m: 1) */
    double acutoff;   /* a row switches when its exchange value is below this (reference: -sqrt(eps)) */
} ace_aopt_cfg;
void ace_aopt_cfg_default(ace_aopt_cfg* cfg);   /* 5, kappa = 1, -sqrt(eps) */
size_t ace_aopt_workspace_size(int designs, int P, int n, int nrows_max);
int ace_aopt_select_batch(const ace_aopt_cfg* cfg, int designs, int P, int n, int nrows_max, const double* F,
                          const int32_t* nrows, const int32_t* init, int32_t* rowlist, double* acrit, int32_t* iters,
                          int32_t* switches, uint32_t* status, double* Minv_out, void* workspace,
                          size_t workspace_bytes, void* stream);
int ace_aopt_select_host(const ace_aopt_cfg* cfg, int designs, int P, int n, int nrows_max, const double* F,
                         const int32_t* nrows, const int32_t* init, int32_t* rowlist, double* acrit, int32_t* iters,
                         int32_t* switches, uint32_t* status, double* Minv_out);   /* host arrays; allocates, copies, synchronous */

/* ---- nuclear-norm prox (A2nuclear ArgMinZ / Shrink) ---------------------------------------
 *   Z = U * Shrink(S, tau) * V'  with [U,S,V] = svd(E)     inferLowRank_Nuclear.m:411-439
 * for a batch of n x r matrices E_b (DEVICE, c128, [batch][r][n]: column j of E_b at
 * E + 2*(b*r + j)*n doubles), r <= 32, tau > 0: the r-general Z-prox kernel of the A2nuclear
 * stages (singular values through the r x r Gram matrix and the Jacobi eigensolver).  Exposed for
 * the prox's own known-answer test; asynchronous on `stream`. */
int ace_nuclear_prox_batch(int batch, int n, int r, const double* E, double tau, double* Z, void* stream);

/* Synthetic traces (device).  Counter-based RNG (splitmix64 of seed/stream/counter),
 * identical integer streams to ace_amd.synth on the host.
 *   ace_synth_codebook: A[count][m][n] c128 with entries exp(j*pi/2*k)/sqrt(n),
 *     k ~ U{0..3}; realisation index base `first` (private A) -- for a shared codebook
 *     pass count = 1, first = -1.
 *   ace_synth_channels: for realisations first..first+count-1: vecH [count][n] c128
 *     (L paths, AoD/AoA ~ U(-47.5deg, 47.5deg), CN gains normalised), B = |A vecH + w|
 *     with w ~ CN(0, 10^(-snr_db/10)), and X0 = vecH + x0_noise * ||vecH||/sqrt(n) * CN(0,1).
 *     A is [a_shared?1:count][m][n]. */
int ace_synth_codebook(uint64_t seed, int64_t first, int count, int m, int n, double* A, void* stream);
int ace_synth_channels(uint64_t seed, int64_t first, int count, int m, int tx, int rx, int L,
                       double snr_db, double x0_noise, const double* A, int a_shared,
                       double* vecH, double* B, double* X0, void* stream);

/* ---- the reference's Monte-Carlo scenarios (Generate_Channel.m:64-142, Generate_Measurement.m:67-118) ----------
 * ace_synth_scenario draws, for the realisations first .. first + count - 1, the channel and every measurement kind
 * the programs under Numerical_Simulation/main_programs use, each at its own scale and without a host round trip:
 *   channel  L dominant paths with AoD, AoA ~ U(-search_deg/2, search_deg/2) (fix_angle: 0 and 15 degrees), snapped
 *            in sin to the grid linspace(-1,1,NQ+1)(1:end-1) with on_grid (nearest point, the first on a tie), unit-norm
 *            CN gains; with L == 1, rician_k further paths with angles ~ U(-pi/2, pi/2) and unit-norm CN gains, mixed as
 *            H = sqrt(K/(K+1)) H_dominant + sqrt(1/(K+1)) H_nlos, K = 10^(k_factor_db/10) (rician_k is ignored for
 *            L > 1, as in the reference).  vecH [count][n] c128, n = tx rx, entry r + rx t = H[r][t].
 *   measure  y = A vecH + noise; noise_model 0: iid CN(0, sigma2) per probe, sigma2 = 10^(-snr_db/10) (the model of
 *            ace_synth_channels); noise_model 1: the reference's diag(W' * noiseMatrix) repeated per transmit beam,
 *            noise(it Mr + q) = sum_r conj(W[q][r]) N[r][q], N iid CN(0, sigma2), W [Mr][rx] c128 the combiners as
 *            ace_beam_scan_batch takes them (m = Mt Mr, probe i = it Mr + q).  add_noise = 0: y = A vecH (the
 *            reference then reports noise_power 1e-10).  y_noisy = y .* CN(0,1) (measurements_with_noisy_phase),
 *            B_raw = |y|, scale = ||B_raw||.
 *   scaled   B = B_raw / scale, X0 = (vecH + x0_noise ||vecH|| / sqrt(n) CN(0,1)) / scale, Hn = vecH / scale: what
 *            ace_synth_channels returns; zeros, not NaN, for a realisation with scale == 0.
 *   paths    [count][4 (L + Rk)] f64, Rk = rician_k if L == 1 else 0: AoD [L] and AoA [L] in degrees, gains [2L]
 *            (re, im; unit norm, before the K-factor weights), NLOS AoD [Rk] and AoA [Rk] in radians, NLOS gains [2Rk].
 * Random streams (counter generator of ace_synth_*; kind + 16 (realisation + 1)): 2 angles, 3 gains, 4 iid noise
 * (counter = probe), 5 X0 -- so the default cfg draws ace_synth_channels' numbers -- and 10 NLOS angles, 11 NLOS gains,
 * 12 phase noise (counter = probe), 13 combiner noise matrix (counter = q rx + r).
 * All pointers are DEVICE pointers; A is [a_shared ? 1 : count][m][n] c128; every output may be NULL and the others do
 * not depend on which are.  A realisation's outputs are a function of (cfg, seed, its index, A, W) alone: not of
 * count or of its place in the call.  With a shared A the product runs on the f64 matrix cores over the whole call
 * (csrc/ace_scenario.hip); no atomics, every sum has a fixed order.  Asynchronous on `stream`, reads nothing back, can
 * be captured.  workspace: ace_synth_scenario_workspace_size(...) bytes of DEVICE memory (0 outside the limits);
 * ACE_ERR_WORKSPACE when NULL or shorter.
 * Limits: 1 <= tx, rx <= 32, 1 <= m <= 4096, 1 <= L <= 8, 0 <= rician_k <= 16, 0 <= NQt, NQr <= 65536
 * (ACE_ERR_UNSUPPORTED above, ACE_ERR_ARG below); count < 1, first < 0, fix_angle with L > 1, a noise_model other than
 * 0 / 1, noise_model 1 without W or with Mr < 1 or m % Mr != 0, a search_deg outside (0, 180], a non-finite snr_db or
 * k_factor_db, x0_noise < 0, ant_d or lambda not positive and finite, and a NULL cfg or A return ACE_ERR_ARG; all of it
 * before any HIP call. */
typedef struct ace_scenario_cfg {
    int L;              /* dominant paths, 1..8 */
    int rician_k;       /* NLOS paths; used only when L == 1 (Generate_Channel.m: forced to 0 for L > 1), 0..16 */
    int on_grid;        /* snap the dominant AoD/AoA to linspace(-1,1,NQ+1)(1:end-1) in sin, first on a tie */
    int fix_angle;      /* AoD = 0, AoA = 15 deg; needs L == 1 */
    int NQt, NQr;       /* grid sizes for on_grid; 0 = 4 * antennas */
    int add_noise;      /* 0: y = A h, reported noise_power 1e-10 (Add_Noise_Flag = 0) */
    int noise_model;    /* 0 iid CN(0, sigma2) per probe (the synth's); 1 the reference's W' * noiseMatrix */
    double search_deg;  /* Searching_Area: AoD, AoA ~ U(-search_deg/2, search_deg/2) */
    double k_factor_db; /* 7 */
    double snr_db, x0_noise, ant_d, lambda;
} ace_scenario_cfg;
void ace_scenario_cfg_default(ace_scenario_cfg* cfg);   /* L 3, rician_k 0, 95 deg, iid, 30 dB, 0.5: ace_synth_channels' scenario */
size_t ace_synth_scenario_workspace_size(const ace_scenario_cfg* cfg, int count, int m, int tx, int rx, int Mr);
int ace_synth_scenario(const ace_scenario_cfg* cfg, uint64_t seed, int64_t first, int count, int m, int tx, int rx,
                       const double* A, int a_shared, const double* W, int Mr,
                       double* vecH, double* y, double* y_noisy, double* B_raw, double* scale,
                       double* B, double* X0, double* Hn, double* paths,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- kernel timing (measurement only; no reference counterpart) ----------------
 * Between ace_prof_start and ace_prof_stop every kernel ace_admm_solve_batch
 * enqueues is bracketed by a pair of hipEvents recorded on the launch stream.
 * ace_prof_stop waits for the events and returns, per kernel class, the summed
 * device time (ms) and the number of launches.  Process-global; not thread-safe. */
#define ACE_K_SETUP 0    /* K = A A^H, (I+K)^{-1}, A^H */
#define ACE_K_INIT 1     /* A X0, init, initial Z-prox, K Y */
#define ACE_K_PRE 2      /* V = Z - N/mu, S = Y - M/mu */
#define ACE_K_APPLY_A 3  /* T = S - A V */
#define ACE_K_APPLY_G 4  /* g = G T */
#define ACE_K_YSTEP 5    /* ArgMinY, M update, reductions */
#define ACE_K_APPLY_K 6  /* K Y */
#define ACE_K_APPLY_AH 7 /* X = V + A^H g */
#define ACE_K_ZSTEP 8    /* ArgMinZ, N update, residuals, stop test */
#define ACE_K_FINAL 9
#define ACE_K_MSR 10     /* m-space run: several steady iterations of the unit in one launch */
#define ACE_NKCLASS 11
int ace_prof_start(int max_launches);
/* From the next ace_prof_start on, record only every stride-th launch of each kernel class
 * (default 1) except the classes whose bit (1 << ACE_K_*) is set in full_mask, which are
 * recorded on every launch: keeps the event overhead out of a throughput measurement. */
int ace_prof_sample(int stride, uint32_t full_mask);
int ace_prof_stop(double* total_ms, int32_t* launches);
/* Realisation-iterations the unit solves between the last ace_prof_start / ace_prof_stop pair
 * settled in m-space form (RealState::msp: no apply_AH pass, no Z traffic), for the bench's
 * per-launch work accounting. */
int ace_prof_msp_steps(long long* steps);
/* Fresh-reference diagnostics of the last unit solve run with ACE_RECERT_TRACE=1 in the environment: out[0] requests
 * for a fresh certificate reference (RealState::recert) the one-wave Z-step honoured, out[1] those whose exact Ky Fan
 * certificate failed (the eigensolver ran), out[2] the iteration at which the first m-space run started (0: none).
 * ACE_ERR_ARG when no such solve has run.  One solve at a time: not for concurrent solves. */
int ace_recert_stats(int32_t* out);
/* Algorithmic flops (8 per complex multiply-add) of the launches the last ace_prof_start /
 * ace_prof_stop pair recorded, per kernel class: the GEMM-shaped applies and prox steps of the
 * f64 path (pipeline stages, PhaseLift) carry their count; classes the caller accounts for
 * itself (the unit path's fused kernels) report 0.  flops: [ACE_NKCLASS]. */
int ace_prof_work(double* flops);
/* The same per kernel class, with the launches' algorithmic HBM bytes (every array the step needs read
 * or written once) and int8 matrix-core ops beside the flops; any pointer may be NULL.  Every class
 * of the pipeline's r-column stages (the int8 digit-plane applies, the r-column Z-step, the Y-step,
 * the pre-pass) carries its bytes, so the dominant class by device time has a roofline. */
int ace_prof_work_ex(double* flops, double* bytes, double* int8_ops);

/* InferADMM solves (unit solves and every pipeline stage) per apply path since the last reset,
 * process-wide: counts[0] shared phase-code codebook on the exact int8 digit-plane applies,
 * counts[1] private phase-code codebooks (2-bit code images), counts[2] f64 applies on a shared
 * A, counts[3] f64 applies on private A.  reset != 0 zeroes the counters after reading them;
 * counts may be NULL.  Tells a caller whether its codebook reached the phase-code path. */
int ace_path_counts(int64_t* counts, int reset);

/* Dynamic LDS (bytes) the launcher of `kernel` requests at operand size `m` (host arithmetic, no
 * GPU call): "i8ah" (apply_AH), "i8ah_fuse", "i8ah_ky" (K Y), "gyk", "gyf", "msr", "nms" (m = the
 * measurement count), "hetrd", "hetrd_blk" (m = the Hermitian order), "scan" (the beam scan; m is not used), "receval" / "receval_rect" (the recovery evaluator,
 * square / rectangular arrays; m = max(tx, rx)),
 * "omp", "gamp" (m = d, the atoms' length), "prgamp" (m = the measurement count), "minl2" (m = the measurement count; 0 at every m).  With the kernel's static LDS
 * (compiler resource report) it must stay within the CU's 160 KiB for every shape the path takes;
 * tests/test_lds_budget.py checks that.  ACE_ERR_ARG for an unknown name. */
int ace_lds_request(const char* kernel, int m, size_t* bytes);

/* Last error text for this thread ("" if none). */
const char* ace_last_error(void);

/* Library version string. */
const char* ace_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ACE_H_ */
