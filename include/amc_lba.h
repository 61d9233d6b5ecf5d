/*
 * amc_lba.h — C ABI of the MI355X-native continuous-time (GP) local bundle adjustment.
 *
 * This is the drop-in boundary for AMC-SLAM's local BA hot path.  The reference builds a
 * g2o::SparseOptimizer inside Optimizer::LocalGPBA (src/Optimizer.cc:713-1432, declared at
 * include/Optimizer.h:58) and calls SparseOptimizer::optimize (Thirdparty/g2o/g2o/core/
 * sparse_optimizer.cpp:354-419).  A caller using this library keeps LocalGPBA's window
 * selection and post-pass, fills the flat arrays below instead of g2o vertices/edges, and
 * calls lba_optimize().  Plain C types only; every array is caller-owned and copied.
 *
 * Conventions (mirroring g2o):
 *   - Tangent order is Sophus [translation; rotation]; pose update T <- T*exp(d)
 *     (src/G2oTypes.cc:41-46), velocity and landmark updates are additive.
 *   - Quaternions are stored (x, y, z, w) like Eigen::Quaternion::coeffs().
 *   - Hessian vertex order: non-fixed keyframes in array order, then landmarks in array
 *     order (g2o sorts active vertices by id and puts non-marginalized first,
 *     sparse_optimizer.cpp:166-190).  Callers that want g2o's exact ordering pass
 *     keyframes sorted by mnId.
 *   - b = -sum J^T rho' Omega e, H dx = b (base_multi_edge.hpp:35-48, 170-222).
 *   - Status codes: >= 0 success (lba_optimize: iterations run), LBA_E_* < 0 on error.
 */
#ifndef AMC_LBA_H
#define AMC_LBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LBA_ABI_VERSION 5   /* 5: lba_solver_info writes out[8] (was out[5]) */

/* status codes */
#define LBA_OK              0
#define LBA_E_EMPTY        -1   /* empty graph: no edges or no free vertices (sparse_optimizer.cpp:358-361) */
#define LBA_E_SOLVE        -2   /* reduced-camera factorisation not positive (linear_solver_dense.h:108-112) */
#define LBA_E_DIVERGED     -3   /* LocalGPBA divergence guard (src/Optimizer.cc:1354-1358), set by host adapter */
#define LBA_E_ARG          -4   /* invalid argument / malformed problem */
#define LBA_E_HIP          -5   /* HIP runtime error */
#define LBA_E_LIMIT        -6   /* problem exceeds a compiled limit (see lba_last_error) */
#define LBA_E_TIMEOUT      -7   /* a bounded device hand-off wait gave up (never expected: e.g. a GPU shared with
                                   another launch that keeps workgroups from being scheduled); the results are not
                                   used and the problem's state is undefined until the next lba_set_problem */

/* observation kinds (the reprojection edges of include/G2oTypes.h) */
#define LBA_MONO_GP    0   /* EdgeMonoGPExtrinsic / EdgeMonoGP: 2-d, vertices (kf_a=prev KF, kf_b=KF, lm, the camera extrinsic: optimised when lba_cam.ext_free)
                              (include/G2oTypes.h:292-402, src/G2oTypes.cc:225-367) */
#define LBA_STEREO_GP  1   /* EdgeStereoGP: 3-d [u, v, u_r] (include/G2oTypes.h:404-421, src/G2oTypes.cc:369-443) */
#define LBA_MONO       2   /* EdgeMono: 2-d, vertices (kf_b, lm) at KF time (include/G2oTypes.h:423-446, src/G2oTypes.cc:445-468) */
#define LBA_STEREO     3   /* EdgeStereo: 3-d (include/G2oTypes.h:448-468, src/G2oTypes.cc:470-495) */

/* lba_config.flags.  Timing inserts HIP events into the stream (each costs a few us of
 * device idle time), so both are off by default. */
#define LBA_FLAG_TIME_SWEEP   1   /* time every launch of the residual/Jacobian sweep kernel
                                     (lba_stats.ms_k_linearize) */
#define LBA_FLAG_TIME_PHASES  2   /* also time every phase (ms_linearize .. ms_update_eval); runs the
                                     host-driven loop */
#define LBA_FLAG_HOST_LOOP    4   /* take every LM decision on the host, one trial at a time (default:
                                     the trials are queued and decided on the device; same results) */
#define LBA_FLAG_BAND_SOLVE   8   /* solve the reduced camera system by forward / back substitution after
                                     the factorisation instead of through the tiles of L^-1 (default:
                                     chosen by size; large pose systems always take this path) */
#define LBA_FLAG_DENSE_SOLVE 16   /* force the L^-1-tile solve (pose systems up to 6144 only) */
#define LBA_FLAG_TIME_SAMPLED 32  /* with LBA_FLAG_TIME_SWEEP in the queued loop: events on one trial in
                                     ten (the 6th of each ten of a batch), so their idle time costs ~1/10 */
#define LBA_FLAG_SUBTREE_SOLVE 64 /* partitioned problems: distributed factorisation of the reduced camera
                                     system (each rank factors its subtree of the nested dissection, the ranks
                                     sum their contributions to the top separators, every rank factors the
                                     top); the window must be split by lba_partition_assign */
#define LBA_FLAG_F32_RESIDUAL 128 /* the fp32-residual option of BASELINE configs[4] ("fp32 residuals + fp64
                                     accumulate"): each observation's projection, residual and Jacobian rows in
                                     fp32 (the world offset Xw - twb in fp64), the robust weights and every sum of
                                     H / b, the Schur complement and the solve in fp64; results within fp32
                                     rounding of the fp64 path, not bitwise */

/* LM termination codes in lba_stats.result (OptimizationAlgorithm::SolverResult) */
#define LBA_RESULT_OK         0
#define LBA_RESULT_TERMINATE  1
#define LBA_RESULT_STOPPED    2   /* stop flag raised (SparseOptimizer::terminate) */

typedef struct lba_config {
    double qc[36];          /* GaussianProcess::mQc, 6x6 row-major (Tracking.cc:753-758 builds diag(Gaussian.Qc)) */
    double huber_mono;      /* Huber delta for 2-d edges; LocalGPBA: (double)(float)sqrt(5.991)  (Optimizer.cc:975) */
    double huber_stereo;    /* Huber delta for 3-d edges; (double)(float)sqrt(7.815)           (Optimizer.cc:977) */
    double huber_prior;     /* Huber delta on EdgeGaussianPrior; <= 0: none (LocalGPBA), 21.026 in BundleAdjustment (:99-136) */
    double lambda_init;     /* OptimizationAlgorithmLevenberg userLambdaInit; <= 0 -> tau * max diag (levenberg.cpp:171-185) */
    double tau;             /* 1e-5 (levenberg.cpp:47) */
    int    max_trials;      /* _maxTrialsAfterFailure, 10 (levenberg.cpp:51) */
    int    early_stop;      /* 1: g2o stop rules active (3 iterations of <1e-3 gain, levenberg.cpp:157-166); 0: fixed count */
    int    device;          /* HIP device ordinal */
    int    flags;           /* LBA_FLAG_* bits, 0 for production use */
} lba_config;

typedef struct lba_kf {     /* VertexPoseVel / PoseVelocity (include/G2oTypes.h:59-80,104-126) */
    double q[4];            /* Twb rotation (x,y,z,w) */
    double t[3];            /* Twb translation */
    double vel[6];          /* PoseVelocity::Vel, world-frame twist [v; w] */
    double time;            /* PoseVelocity::time (KF time stamp) */
    double bf;              /* PoseVelocity::bf (stereo baseline * fx) */
    int32_t fixed;          /* vertex fixed (no Hessian rows) */
    int32_t pad;
} lba_kf;

typedef struct lba_obs {
    int32_t kind;           /* LBA_MONO_GP .. LBA_STEREO */
    int32_t kf_a;           /* GP kinds: previous KF (vertex 0); non-GP: ignored (-1) */
    int32_t kf_b;           /* GP kinds: KF (vertex 1); non-GP: the KF (vertex 0) */
    int32_t lm;             /* landmark index */
    int32_t cam;            /* camera index (EdgeMono/EdgeStereo use the reference camera = n_cam-1) */
    int32_t pad;
    double  t;              /* observation time (GP kinds: pKFi->mvTimeStamps[c]) */
    double  z[3];           /* u, v, (u_right for stereo) */
    double  w;              /* information weight invSigma2 / unc2 (Omega = w * I) */
} lba_obs;

typedef struct lba_prior {  /* EdgeGaussianPrior(v0 = kf_a older, v1 = kf_b newer), info QiInv(t_b - t_a) */
    int32_t kf_a;
    int32_t kf_b;
} lba_prior;

typedef struct lba_cam {    /* GeometricCamera (Pinhole) + MultiKeyFrame::mTbc[c] */
    double q[4];            /* Tbc rotation (x,y,z,w) */
    double t[3];            /* Tbc translation */
    double fx, fy, cx, cy;  /* Pinhole::mvParameters (float values widened) */
    /* extrinsic calibration (LocalGPBA bExtrinsic, src/Optimizer.cc:982-995,1228-1240): ext_free = 1
     * makes this camera's VertexExtrinsic (include/G2oTypes.h:83-102, T <- T exp(d)) optimisable.  Its
     * 6 dofs follow the keyframes' in the pose system (g2o id order: iniMPid + c + 1 > every KF id);
     * the LBA_MONO_GP observations of the camera (EdgeMonoGPExtrinsic, src/G2oTypes.cc:241-314) link it,
     * and an EdgeExtrinsicPrior (include/G2oTypes.h:470-494) e = log(Rbc_ini^-1 Rbc), information
     * rbc_info, is attached to it.  0: fixed, as in every call without bExtrinsic (the prior is then
     * inactive: all its vertices are fixed).  Not with a partitioned problem (LBA_E_LIMIT), and an
     * LBA_STEREO_GP observation of such a camera is rejected (EdgeStereoGP projects through the static
     * MultiKeyFrame::mTbc, not the vertex). */
    int32_t ext_free;
    int32_t pad;
    double  rbc_ini[4];     /* MultiFrame::mRbc_ini[c] (x,y,z,w), float values widened (Frame.cc:181) */
    double  rbc_info[9];    /* MultiFrame::mRbc_ini_cov[c] used as the information, row-major (0.2 I, Frame.cc:182) */
} lba_cam;

typedef struct lba_stats {
    int32_t iterations;     /* LM iterations run (SparseOptimizer::optimize return) */
    int32_t trials;         /* total LM trials (sum of qmax) */
    int32_t result;         /* LBA_RESULT_* of the last iteration */
    int32_t solve_failures; /* trials whose factorisation was not positive */
    double  chi2_initial;   /* activeRobustChi2 before the first iteration */
    double  chi2_final;     /* activeRobustChi2 of the last computed errors (g2o semantics) */
    double  lambda_final;
    double  ms_linearize;   /* device time per phase, summed (HIP events; LBA_FLAG_TIME_PHASES):
                               ms_linearize the fused linearisation + landmark elimination of every
                               trial, ms_schur the pose-sample expansion + assembly of S */
    double  ms_schur;
    double  ms_solve;
    double  ms_update_eval;
    double  ms_total;       /* host wall time of lba_optimize */
    double  ms_k_linearize; /* device time of the fused sweep kernel (residual / Jacobian / J^T W J and the
                               landmark elimination, k_lin_schur), summed over its dispatches
                               (LBA_FLAG_TIME_SWEEP or LBA_FLAG_TIME_PHASES) */
    int32_t n_k_linearize;  /* launches of that kernel */
    int32_t n_k_solve;      /* launches of the factorisation + solve kernel (k_chol_flow) */
    double  ms_k_solve;     /* its device time, summed (same flags) */
} lba_stats;

typedef struct lba_problem lba_problem;   /* opaque: owns device buffers + stream */

/* lifecycle */
int         lba_create(lba_problem** out, const lba_config* cfg);
void        lba_destroy(lba_problem* p);
const char* lba_last_error(const lba_problem* p);
int         lba_abi_version(void);
/* Engines created by lba_create and not yet destroyed, process-wide (leak checks: the reference
 * builds and frees its g2o optimiser on every call, src/Optimizer.cc:61-367, so a caller that runs one
 * engine per call or per thread must see this return to its previous value). */
int         lba_live_problems(void);

/* Replace the configuration (Huber deltas, lambda0, Qc, flags) of an existing problem, e.g. between
 * LocalGPBA calls with and without bLarge (OptimizationAlgorithmLevenberg::setUserLambdaInit,
 * RobustKernelHuber::setDelta).  Takes effect at the next lba_set_problem; the device cannot change. */
int lba_set_config(lba_problem* p, const lba_config* cfg);

/* Copy a window to the device (replaces SparseOptimizer::addVertex/addEdge +
 * initializeOptimization, sparse_optimizer.cpp:197-267).  vel_kfs lists the KFs carrying an
 * EdgeVelocity (info QcInv(2,2), Optimizer.cc:858-870).  The arrays may come in any order: fixed
 * keyframes anywhere, kf_a any other keyframe of the window (not only the array neighbour), edges on
 * fixed keyframes (an edge whose vertices are all fixed is inactive).  A vertex no active edge touches
 * (a landmark without an observation, a free keyframe without an edge) is inactive like in g2o: it has
 * no rows in H / b / dx, which are compressed to the active vertices in array order, and its state is
 * never changed.  Keyframe quaternions are normalised on the way in like the Sophus cast (as in
 * lba_set_state), so lba_get_state returns a fixed or inactive keyframe's t and vel bit for bit as
 * passed and its q normalised; an inactive landmark comes back bit for bit. */
int lba_set_problem(lba_problem* p,
                    const lba_kf* kfs, int32_t n_kf,
                    const double* lm_xyz, int32_t n_lm,
                    const lba_obs* obs, int32_t n_obs,
                    const lba_prior* priors, int32_t n_priors,
                    const int32_t* vel_kfs, int32_t n_vel,
                    const lba_cam* cams, int32_t n_cam);

/* ---- partitioned global BA (BASELINE config 4): one problem per GPU (rank), every
 * rank holding ALL keyframes (same array, same fixed flags), a disjoint subset of the landmarks with
 * all of their observations, and rank 0 alone the motion-prior / velocity edges.  Per LM trial the
 * ranks sum their reduced camera systems (the envelope of S, the reduced rhs and b_p: one
 * all-reduce) and their trial sums (chi2 before / after, computeScale: a 4-double all-reduce); every
 * rank then solves the same system, so the keyframe states and the LM decisions stay identical and
 * each rank back-substitutes its own landmarks.  The all-reduce is the caller's (sum, in place, on
 * device memory, enqueued on the given HIP stream, bitwise identical on every rank): RCCL over
 * xGMI (lba_set_partition_rccl), an in-process group of problems on one device (lba_group, for
 * tests), or any function.  Call before lba_set_problem; set_problem is then collective (the ranks
 * agree on the union envelope of S), as are lba_optimize calls, which need lambda_init > 0 and the
 * same iteration count and stop flag on every rank.  A set_problem that fails on one rank fails on
 * every rank: the ranks exchange their set-up status in one all-reduce before the first collective
 * (the others return LBA_E_ARG, "another rank of the partition failed its set-up").  An lba_group
 * rank waits at most 120 s for its peers, then the group is poisoned (every call returns an error). */
typedef int (*lba_allreduce_fn)(double* dev_buf, int64_t count, void* hip_stream, void* user);
int lba_set_partition(lba_problem* p, int32_t rank, int32_t nranks, lba_allreduce_fn fn, void* user);
int lba_rccl_unique_id(void* id_out);   /* NCCL_UNIQUE_ID_BYTES (128) bytes, on one rank, shared by the caller */
int lba_set_partition_rccl(lba_problem* p, const void* id, int32_t rank, int32_t nranks);
typedef struct lba_group lba_group;     /* in-process all-reduce across problems on one device */
int  lba_group_create(lba_group** out, int32_t nranks);
void lba_group_destroy(lba_group* g);
int  lba_set_partition_group(lba_problem* p, lba_group* g, int32_t rank);
/* The landmark / edge split of a window for LBA_FLAG_SUBTREE_SOLVE (host only, no device): the reduced camera
 * system's nested dissection (the plan lba_set_problem makes) is cut into nranks subtrees and the top; each
 * landmark goes to the rank whose subtree holds its keyframes (a landmark that only sees top keyframes, or
 * fixed ones: rank = index mod nranks), each motion prior / velocity edge likewise.  Every rank then holds all
 * keyframes, its landmarks with all their observations, and its edges (the replacement of the l mod N split of
 * lba_set_partition, BlockSolver's Schur complement per partition, block_solver.hpp:381-445).  Outputs
 * lm_rank[n_lm], prior_rank[n_priors], vel_rank[n_vel]; panels_out (may be NULL) [3]: panels of the system,
 * panels in the top, columns of the largest subtree; kf_rank (may be NULL) [n_kf]: the rank whose subtree holds
 * the keyframe (-1: the top, or fixed).  Cameras are not an input: a partitioned lba_set_problem rejects free
 * extrinsics (lba_cam.ext_free, LBA_E_LIMIT) before it plans, so the pattern planned here (keyframe blocks only)
 * is the one every partitioned set-up factors. */
int lba_partition_assign(const lba_config* cfg, const lba_kf* kfs, int32_t n_kf, int32_t n_lm, const lba_obs* obs,
                         int32_t n_obs, const lba_prior* priors, int32_t n_priors, const int32_t* vel_kfs, int32_t n_vel,
                         int32_t nranks, int32_t* lm_rank, int32_t* prior_rank, int32_t* vel_rank, int32_t* panels_out,
                         int32_t* kf_rank);
/* LBA_FLAG_SUBTREE_SOLVE: per keyframe slot, the rank whose subtree holds it (-1: the top, every rank holds its
 * state; a keyframe of another rank's subtree keeps its old state on this rank: gather it from its owner). */
int  lba_kf_owner(const lba_problem* p, int32_t* owner);
/* The rank's share of the factorisation: out[0] its factorisation FLOPs (its subtree's columns + the top; the
 * whole system when the solve is replicated), out[1] the whole system's, out[2] bytes it all-reduces per LM trial
 * for the solve (split: the top tiles + bS + b_p; replicated: every tile + bS + b_p; 0 unpartitioned), out[3]
 * the replicated solve's bytes for comparison, out[4] panels of its subtree, out[5] panels of the top. */
int  lba_split_info(const lba_problem* p, double out[6]);

/* ---- window farm (BASELINE config 3): one LocalGPBA window per GPU (rank), windows cut
 * from one trajectory, so neighbours share keyframes and map points.  The reference runs one local BA at
 * a time (LocalMapping::Run -> Optimizer::LocalGPBA, src/LocalMapping.cc:131) and every window reads and
 * writes the shared map (src/Optimizer.cc:1380-1432); here the shared estimates are exchanged at window
 * boundaries instead, device to device:
 *   lba_set_farm*      the collective: RCCL over xGMI (lba_set_farm_rccl: ncclAllGather on the problem's
 *                      stream), an in-process group on one device (lba_set_farm_group, for tests), or any
 *                      sum all-reduce of the caller's (an all-gather as a sum over zero-padded slots);
 *   lba_farm_plan      after lba_set_problem, collective: which vertices this rank publishes (owner ==
 *                      rank) and, for every vertex another rank owns, where its estimate lands in the
 *                      exchange buffer (matched by global id once; no lookups at exchange time);
 *   lba_farm_exchange  collective, per window boundary: pack kernel -> all-gather -> unpack kernel on the
 *                      problem's stream; the received estimates are bit-exact copies of the owners'.
 * kf_owner / lm_owner: per vertex of this window, the rank that publishes it, or -1 for a vertex no other
 * window shares.  Keyframe time stamps and fixed flags are not exchanged (they are the same everywhere).
 * A vertex whose owner does not publish it (no such global id on that rank) keeps its own estimate; the
 * counts of published, received and unmatched vertices come back in out_counts[5] (may be NULL):
 * kf published, lm published, kf received, lm received, unmatched.  lba_set_problem drops the plan. */
int lba_set_farm(lba_problem* p, int32_t rank, int32_t nranks, lba_allreduce_fn fn, void* user);
int lba_set_farm_rccl(lba_problem* p, const void* id, int32_t rank, int32_t nranks);
int lba_set_farm_group(lba_problem* p, lba_group* g, int32_t rank);
int lba_farm_plan(lba_problem* p, const int64_t* kf_gid, const int32_t* kf_owner,
                  const int64_t* lm_gid, const int32_t* lm_owner, int32_t* out_counts);
int lba_farm_exchange(lba_problem* p);
/* Host-only form of the plan's matching (no device, no collective; tests): given every rank's published
 * global ids (pub_gid: nranks x cap, -1 padded) and this window's ids / owners, the source slot of every
 * received vertex: src[i] = owner * cap + position, or -1 (not a received vertex, or unmatched). */
int lba_farm_match(int32_t rank, int32_t nranks, int32_t cap, const int64_t* pub_gid,
                   const int64_t* gid, const int32_t* owner, int32_t n, int32_t* src);

/* Levenberg-Marquardt (OptimizationAlgorithmLevenberg::solve x iters).  stop_flag is polled
 * between iterations and trials like SparseOptimizer::terminate().  Returns iterations run
 * (>= 0) or an LBA_E_* code. */
int lba_optimize(lba_problem* p, int32_t iters, volatile const int32_t* stop_flag, lba_stats* out);

/* write-back: current (accepted) estimates */
int lba_get_state(lba_problem* p, lba_kf* kf_out, double* lm_out);
/* overwrite the current estimates (window-boundary exchange of shared keyframes/landmarks in a
 * multi-GPU window farm); either pointer may be NULL to keep that part.  Quaternions are
 * re-normalised like the Sophus cast. */
int lba_set_state(lba_problem* p, const lba_kf* kf_in, const double* lm_xyz);

/* Errors of the current estimate: robust chi2 sum, per-observation chi2 (e^T Omega e) and
 * the LocalGPBA depth test (both KF poses for GP edges, include/G2oTypes.h:305-314).
 * Any output pointer may be NULL. */
int lba_eval(lba_problem* p, double* chi2_robust, double* obs_chi2, uint8_t* depth_ok);
/* Per-observation chi2 of the last computed errors, without evaluating anything: after lba_optimize
 * the errors of its last trial state, accepted or not (g2o's e->chi2() after optimize(): the
 * _error of the last computeActiveErrors, src/Optimizer.cc:1300-1330). */
int lba_trial_chi2(lba_problem* p, double* obs_chi2);

/* Parity/debug entry points (no LM).  lba_linearize: computeActiveErrors + buildSystem at the
 * current estimate: residuals [n_obs*3] (unused components 0), H_pp dense [np*np] full
 * symmetric, b [np + 3*n_lm], H_ll [n_lm*9].  Any pointer may be NULL.  Returns np. */
int lba_linearize(lba_problem* p, double* residuals, double* H_pp, double* b, double* H_ll);
/* One damped solve at lambda on the last linearisation: dx [np + 3*n_lm] (poses then
 * landmarks), BlockSolver::solve with setLambda/restoreDiagonal (block_solver.hpp:354-486). */
int lba_solve_step(lba_problem* p, double lambda, double* dx);
/* The trial state of the last lba_solve_step: the current estimate with that step applied by the device's update
 * (VertexPoseVel / VertexSBAPointXYZ oplus, src/G2oTypes.cc:41-46, sparse_optimizer.cpp:422-435), i.e. what g2o's
 * LM evaluates after push() + update() (optimization_algorithm_levenberg.cpp:94-103); the current estimate is not
 * changed.  Same layout as lba_get_state. */
int lba_trial_state(lba_problem* p, lba_kf* kf_out, double* lm_out);
/* Diagnostics: the host preprocessing of lba_set_problem alone (device order, pairs, tiles, slabs; no device,
 * no GPU needed) on the given window; phase_ms: wall ms of the order/pairs, tiles and slots/state phases;
 * counts: device landmarks, pose blocks, pose dimension, tiles, a 32-bit fingerprint of the tiling and slab
 * layout (the same for any LBA_SETUP_THREADS).  Returns LBA_OK or the error lba_set_problem would return. */
int lba_setup_host_profile(const lba_config* cfg, const lba_kf* kfs, int32_t n_kf, const double* lm_xyz, int32_t n_lm,
                           const lba_obs* obs, int32_t n_obs, const lba_prior* priors, int32_t n_priors,
                           const int32_t* vel_kfs, int32_t n_vel, const lba_cam* cams, int32_t n_cam,
                           double phase_ms[3], int32_t counts[5]);
/* Diagnostics: the largest tile shapes of the same host preprocessing (no device): the work sizes of the sweep's
 * per-tile phases.  shapes[0..8] over the regular (eliminating) tiles: their number, then the maxima of a tile's
 * observations, Jacobian rows, pose samples, rows of one pose sample, landmarks, (KF, landmark) pairs, KFs and
 * Schur entries; shapes[9..13] over the segment tiles of heavy landmarks: their number, then the maxima of
 * observations, rows, pose samples and pairs.  Returns LBA_OK or the error lba_set_problem would return. */
#define LBA_TILE_SHAPES 14
int lba_setup_tile_shapes(const lba_config* cfg, const lba_kf* kfs, int32_t n_kf, const double* lm_xyz, int32_t n_lm,
                          const lba_obs* obs, int32_t n_obs, const lba_prior* priors, int32_t n_priors,
                          const int32_t* vel_kfs, int32_t n_vel, const lba_cam* cams, int32_t n_cam,
                          int32_t shapes[LBA_TILE_SHAPES]);
/* Diagnostics: `passes` back-to-back parallel passes of lba_set_problem's host thread pool, of 1..max_pieces
 * pieces each (short and long passes alternating); returns the number of pieces that did not run exactly once
 * in their own pass or were still running when their pass returned (0 when the pool is sound).  No device. */
int lba_debug_pool_stress(int32_t passes, int32_t max_pieces);
/* Diagnostics: the Lie-group primitives of the kernels (Sophus SE3 exp / log, Thirdparty/Sophus/sophus/se3.hpp:
 * 223-252,761-781; RightJacobianPose3 / RightJacobianPose3Inv, src/Pose3utils.cc:5-46, small-angle branches
 * included) evaluated on `device` for n records in[13 n] = {xi[6], q[4] (x,y,z,w), t[3]}: out[85 n] =
 * {exp(xi) q[4] t[3], log(q, t)[6], Jr(xi)[36], Jr^-1(xi)[36]} (row-major). */
int lba_debug_lie(int32_t device, int32_t n, const double* in, double* out);
/* Diagnostics: set the problem's device fault word to `code` (1 factorisation, 2 assembly, 4 trial evaluation:
 * the waits of one launch that gave up), as a bounded in-launch wait does when it times out.  The next call that
 * reads the word (lba_optimize, lba_linearize, lba_solve_step, lba_eval) fails with LBA_E_TIMEOUT and clears it,
 * so the failure path can be tested without a hang.  No LM work. */
int lba_debug_inject_fault(lba_problem* p, int32_t code);
/* How the reduced camera system is solved (after lba_set_problem), at the granularity of panels of
 * CHOL_NB = 32 rows: out[0] panels of the loop-closure tail (rows that reach back to the first panels,
 * ordered last), out[1] panels, out[2] stored 32 x 32 tiles of the factor L (fill-in included), out[3] 1
 * for the substitution (band) solve, 0 for the L^-1-tile solve, out[4] panels on the factorisation's
 * dependent chain (the depth of the elimination tree), out[5] levels of the nested dissection, out[6]
 * tiles of the lower triangle of S (the pattern before fill-in), out[7] fill-in tiles (out[2] - out[6]). */
int lba_solver_info(const lba_problem* p, int32_t out[8]);
/* The launch fusions the set-up chose (diagnostics and tests): out[0] 1 when the trial evaluation runs inside
 * k_update (the whole grid resident at once), out[1] 1 when the pose samples' expansion and the assembly of S
 * run as one launch (k_exp_asm), out[2] 1 for the fp32-residual kernels, out[3] the k_update grid. */
int lba_kernel_modes(const lba_problem* p, int32_t out[4]);
/* Algorithmic FLOPs of one solve of the reduced camera system, from the symbolic structure of L:
 * out[0] the tile factorisation (per column with m tiles below the diagonal: potrf + m trsm + m(m+1)/2
 * trailing tile updates), out[1] the forward and back substitutions. */
int lba_solver_flops(const lba_problem* p, double out[2]);
/* Device memory (bytes) the problem's buffers hold: the reduced system and its factor are packed envelope
 * tiles (O(envelope), not O(npose^2)); the dense H_pp of lba_linearize is allocated only when asked for.
 * LBA_E_ARG (< 0) for a null problem. */
int64_t lba_device_bytes(const lba_problem* p);
/* Wall time (ms) of the last lba_set_problem's phases: [0] activity, GP pairs and landmark order, [1] tiles,
 * [2] slab slots and device-order records, [3] host -> device upload, [4] the solve's layout (envelope plan,
 * flow tasks).  Writes min(n, phases) values and returns that count; LBA_E_ARG for a null problem. */
int lba_setup_phases(const lba_problem* p, double* ms, int32_t n);
/* Dimension of the pose system (12 * number of non-fixed KFs + 6 * number of free extrinsics). */
int lba_pose_dim(const lba_problem* p);
/* Current camera extrinsics (write-back of the VertexExtrinsic estimates, src/Optimizer.cc:1419-1428):
 * the cameras passed to lba_set_problem with Tbc (q, t) replaced by the estimate for free ones. */
int lba_get_cams(lba_problem* p, lba_cam* cams_out);

/* ---- tracking: Optimizer::PoseGPOptimizationFromeLastFrame (src/Optimizer.cc:369-686), SURVEY.md §8(f)3.
 * Per frame: vertices prev (pFrame->mpPrevFrame, fixed = the `fix` argument) and cur (pFrame), the map
 * points fixed; EdgeMonoGPOnlyPose for the asynchronous cameras (LBA_MONO_GP: the GP pose between prev
 * and cur at the camera's time stamp), EdgeMonoOnlyPose / EdgeStereoOnlyPose for the reference camera
 * (LBA_MONO / LBA_STEREO at cur), EdgeGaussianPrior(prev, cur) and EdgeVelocity on both.  Four rounds
 * of optimize(10) on the level-0 edges with re-classification between them (chi2 5.991 mono, 15.6 /
 * 9.8 / 7.815 / 7.815 stereo, x1.5 for points tracked closer than 10 m, depth test), the robust kernel
 * dropped after round 3.  A batch of frames runs as one launch, one workgroup per frame. */
typedef struct lba_track_obs {
    int32_t kind;           /* LBA_MONO_GP, LBA_MONO or LBA_STEREO */
    int32_t cam;            /* mmpKeyToCam[i]; the reference camera (n_cam - 1) for LBA_MONO / LBA_STEREO */
    int32_t outlier;        /* in: pFrame->mvbOutlier[i] (edge level 1); out: the last round's classification */
    int32_t close;          /* mvpMapPoints[i]->mvTrackDepth[cam] < 10 */
    double  t;              /* pFrame->mvTimeStamps[cam] (GP kinds) */
    double  z[3];           /* u, v (, u_right) */
    double  w;              /* invSigma2 / unc2 */
    double  Xw[3];          /* pMP->GetWorldPos() widened to double (fixed) */
} lba_track_obs;

typedef struct lba_track_frame {
    lba_kf  prev;           /* VertexPoseVel(pFrame->mpPrevFrame); prev.fixed = fix.  Not written back */
    lba_kf  cur;            /* VertexPoseVel(pFrame); out: the optimised pose and velocity (SetPose / SetVelocity) */
    int32_t obs0, n_obs;    /* the frame's observations in the batch array */
    int32_t n_good;         /* out: nInitialCorrespondences - nBad, the reference's return value */
    int32_t iterations;     /* out: LM iterations over the rounds */
} lba_track_frame;

typedef struct lba_tracker lba_tracker;   /* device buffers + stream, reused across calls */
int  lba_tracker_create(lba_tracker** out, const lba_config* cfg);   /* qc, Huber deltas, tau, device */
void lba_tracker_destroy(lba_tracker* t);
int  lba_track(lba_tracker* t, lba_track_frame* frames, int32_t n_frames, lba_track_obs* obs, int32_t n_obs,
               const lba_cam* cams, int32_t n_cam);

/* ---- tracking: Tracking::MCRansac's hypotheses (src/Tracking.cc:1939-2002), the step before lba_track.
 * Each hypothesis is one Optimizer::OptimizeVel (src/Optimizer.cc:2364-2447): a 6-d VertexVel (additive update,
 * include/G2oTypes.h:128-145) started at pF1->GetVelocity(), one EdgeVelReproj per matched feature
 * (include/G2oTypes.h:521-547, src/G2oTypes.cc:497-510: Xc = (T exp(v dt) Tbc)^-1 Xw, e = z - project(Xc), no
 * depth test, information w I, Huber delta 5.991), only the LBA_VEL_SET sampled edges at level 0; optimize(iterations)
 * of g2o's Levenberg (tau, max_trials, early_stop of the tracker's lba_config, no user lambda), then computeError()
 * on every edge: inlier iff ||e|| <= threshold (pixels, unweighted; a NaN error is an outlier).  The best
 * hypothesis of a frame is the first with strictly more inliers than every earlier one, starting from 0
 * (Tracking.cc:1978-1984).  The caller draws the triples (std::random_device in the reference) and applies the
 * minMatch rule (Tracking.cc:1987-2001) to n_inliers / inlier.  A batch of frames runs as two launches: one wave
 * per hypothesis, then one per frame for the selection.
 * LBA_E_ARG: null tracker, a camera index out of range, a triple with an index outside [0, n_obs) of its frame or
 * with a repeated index, iterations < 0, a dt that is not finite, observation or hypothesis ranges outside the
 * arrays.  LBA_E_LIMIT: more distinct (cam, dt) pairs in a frame than lba_track's 16 pose samples.  A refused
 * call writes nothing.  n_hyp == 0 for a frame (best_hyp = -1) and n_frames == 0 are valid.  A hypothesis's three
 * edges accumulate in ascending observation index.  hyp_iterations is reported, not reproducible to the count:
 * three edges fit six unknowns exactly, chi2 falls to rounding level and the stop rules then fire on noise. */
#define LBA_VEL_SET 3
typedef struct lba_vel_obs {
    int32_t cam;        /* pF1->mmpKeyToCam[index] */
    int32_t inlier;     /* out: the best hypothesis's vbInliers[i]; 0 when there is none */
    double  dt;         /* pF1->mvTimeStamps[cam] - pF2->mTimeStamp */
    double  z[2];       /* mvKeysUn[index].pt */
    double  w;          /* mvInvLevelSigma2[octave] */
    double  Xw[3];      /* pMP->GetWorldPos() widened */
} lba_vel_obs;
typedef struct lba_vel_frame {
    double  q[4], t[3]; /* pF2->GetPoseW(), (x, y, z, w) */
    double  vel[6];     /* in: pF1->GetVelocity(); out: bestVel, untouched when best_hyp < 0 */
    int32_t obs0, n_obs;
    int32_t hyp0, n_hyp;          /* its triples in `samples`: frame-local obs indices */
    int32_t best_hyp, n_inliers;  /* out: frame-local index or -1; its inlier count or 0 */
} lba_vel_frame;
typedef struct lba_vel_params { double threshold, huber_delta; int32_t iterations, pad; } lba_vel_params;
int lba_track_vel_ransac(lba_tracker* t, lba_vel_frame* frames, int32_t n_frames,
                         lba_vel_obs* obs, int32_t n_obs,
                         const int32_t* samples, int32_t n_hyp,   /* [LBA_VEL_SET * n_hyp] */
                         const lba_vel_params* prm,               /* NULL: 2.0, 5.991, 40 */
                         const lba_cam* cams, int32_t n_cam,
                         double* hyp_vel, int32_t* hyp_inliers, int32_t* hyp_iterations); /* each may be NULL */

/* ---- loop closing: Optimizer::OptimizeSim3 (src/Optimizer.cc:2049-2362) for a batch of candidate pairs (KF1, KF2),
 * as LoopClosing.cc:381 / :597 call it once per BoW candidate.  Per pair one 7-dof VertexSim3Expmap S12
 * (include/OptimizableTypes.h:146-173: left update S <- Sim3(update) S, tangent [omega; upsilon; sigma], sigma
 * zeroed under fix_scale; Sim3(update) with its four branches at eps = 1e-5, Thirdparty/g2o/g2o/types/sim3.h:70-142),
 * the map points fixed, and per correspondence the two 2-d edges in g2o's insertion order:
 *   EdgeSim3ProjectXYZ         e = z1 - project1(Tc1b[cam1] S12      Tc2b[cam2]^-1 X2c)   (OptimizableTypes.h:176-201)
 *   EdgeInverseSim3ProjectXYZ  e = z2 - project2(Tc2b[cam2] S12^-1   Tc1b[cam1]^-1 X1c)   (OptimizableTypes.h:203-229)
 * pinhole in double (src/CameraModels/Pinhole.cpp:35-41), no depth test, information w I, Huber delta
 * (double)(float)sqrt(th2) (:2115, :2234-2236).  The reference differentiates both edges numerically (their
 * linearizeOplus is commented out: base_binary_edge.hpp:147-197, central differences of 1e-9 through oplus); the
 * device uses the analytic Jacobian of the same left update, which that difference quotient equals up to its rounding
 * noise.  Flow (:2285-2361): optimize(5) of g2o's Levenberg (tau, max_trials, early_stop of the
 * tracker's lba_config, no user lambda); a correspondence is dropped when either edge's chi2() of the LAST computed
 * errors (the last LM trial's state, accepted or not) exceeds th2, the survivors lose their robust kernel;
 * n_corr - n_bad < 10 returns 0 with these flags written and S12 untouched; otherwise optimize(n_bad > 0 ? 10 : 5)
 * from a fresh lambda, then the errors are recomputed, a survivor with either chi2 > th2 is flagged too, the others
 * count into n_in, and S12 is written back.  A NaN chi2 is not > th2.  mAcumHessian (zeroed, never filled, :2337) is
 * not exposed; the caller-side filtering of the matches (:2125-2216) is amc_lba.sim3.sim3_rows.
 * A batch is one launch, one workgroup per pair; a pair's result does not depend on the batch or on its position.
 * LBA_E_ARG: null tracker or arrays, n_cam < 1, a pair's correspondence range outside [0, n_corr) or camera range
 * [cam0, cam0 + 2 n_cam) outside [0, n_cam_rows), cam1 / cam2 outside [0, n_cam), th2 not finite or <= 0, s not
 * finite or <= 0.  LBA_E_LIMIT: a pair whose rows and cameras exceed a workgroup's 64 KB of LDS (about 600
 * correspondences with 4 cameras).  A refused call writes nothing.  n_pairs == 0 is valid, and so is n_corr == 0 for
 * a pair (n_in = n_bad = iterations = 0, S12 untouched).  When the correspondence ranges of two pairs overlap, the
 * shared rows carry the flags of the later pair.  A failed 7 x 7 factorisation (non-positive pivot of the unpivoted
 * Cholesky) is a trial with chi2 = max, as in lba_track. */
typedef struct lba_sim3_cam {
    double q[4], t[3];      /* Tcb of this camera of this keyframe, (vT1w[i] * T1bw^-1) widened (:2083-2088); (x, y, z, w) */
    double fx, fy, cx, cy;  /* vpCamera1[i] / vpCamera2[i]: pinhole parameters */
} lba_sim3_cam;
typedef struct lba_sim3_corr {
    int32_t cam1;           /* pKF1->mmpKeyToCam[i] (:2133) */
    int32_t cam2;           /* the first camera of KF2 that sees pMP2 (:2140-2150) */
    int32_t outlier;        /* out: vpMatches1[idx] was set to NULL (:2303, :2350) */
    int32_t pad;
    double  X1c[3];         /* vR1w[cam1] P3D1w + vt1w[cam1], widened (:2163-2165) */
    double  X2c[3];         /* vR2w[cam2] P3D2w + vt2w[cam2], widened (:2171-2173) */
    double  z1[2], z2[2];   /* pKF1->mvKeysUn[i].pt, pKF2->mvKeysUn[i2].pt (:2222-2224, :2246-2247) */
    double  w1, w2;         /* mvInvLevelSigma2[octave] of either keyframe (:2231, :2270) */
} lba_sim3_corr;
typedef struct lba_sim3_pair {
    double  q[4], t[3], s;  /* in: g2oS12 (:2095), (x, y, z, w); out: vSim3_recov->estimate() (:2358-2359), untouched
                               when the early return was taken (n_corr - n_bad < 10, :2328-2329) */
    double  th2;            /* the reference's float th2, widened */
    int32_t fix_scale;      /* bFixScale */
    int32_t corr0, n_corr;  /* its rows of `corr`: nCorrespondences = n_corr */
    int32_t cam0;           /* the first of its 2 n_cam cameras in `cams`: KF1's vTc1b, then KF2's vTc2b */
    int32_t n_in;           /* out: the return value (nIn, or 0 of the early return) */
    int32_t n_bad;          /* out: nBad of the first pass (:2291-2320) */
    int32_t iterations;     /* out: LM iterations of both rounds (reported; near the minimum decided by rounding) */
    int32_t pad;
} lba_sim3_pair;
int lba_sim3_optimize(lba_tracker* t, lba_sim3_pair* pairs, int32_t n_pairs, lba_sim3_corr* corr, int32_t n_corr,
                      const lba_sim3_cam* cams, int32_t n_cam_rows, int32_t n_cam);
/* Measurement only: on != 0 makes lba_sim3_optimize bracket its launch with two events on the tracker's stream;
 * last_ms (may be NULL) receives the kernel time of the last such call in milliseconds, or -1. */
int lba_sim3_profile(lba_tracker* t, int32_t on, double* last_ms);

/* ---- loop closing: the Sim3Solver RANSAC that runs before OptimizeSim3 (src/Sim3Solver.cc, driven by
 * LoopClosing::DetectCommonRegionsFromBoW, src/LoopClosing.cc:527-539) for a batch of candidate pairs.  One call is
 * the whole `while (!bNoMore && !bConverge) iterate(20, ...)` loop of every pair: the caller draws the
 * mRansacMaxIts triples (amc_lba.sim3_ransac.draw_triples, :277-291) and filters the matches
 * (amc_lba.sim3_ransac.sim3_ransac_rows, :85-147).
 * Hypothesis (ComputeSim3, :343-459), in fp64 on the float-valued inputs widened: centroids of the triple's three
 * columns and relative coordinates, M = Pr2 Pr1^T summed in column order, Horn's 4 x 4 symmetric N (:367-381), the
 * eigenvector q = (w, vec) of its largest eigenvalue (a cyclic Jacobi of 6 fixed sweeps); |vec| < 1e-5 is DEGENERATE
 * (quirk b); R12 the rotation of that unit quaternion (the reference's atan2 / SO3::exp route gives the same rotation
 * whatever the sign of q); s12 = sum(Pr1 . R Pr2) / sum((R Pr2)^2), or 1 under fix_scale; t12 = O1 - s R O2;
 * T21 = [(1/s) R^T | -(1/s) R^T t] (:452-458).
 * Scoring (CheckInliers, Project, FromCameraToImage, :462-536): p11 = pi1(Tc1b[cam1] X1b), p22 = pi2(Tc2b[cam2] X2b)
 * (the points' own projections, not keypoints), p21 = pi1(Tc1b[cam1] (s R X2b + t)), p12 = pi2(Tc2b[cam2] T21 X1b);
 * a row is an inlier iff |p11 - p21|^2 < max_err1 AND |p12 - p22|^2 < max_err2, strictly.  Pinhole, no depth test; a
 * non-finite error is an outlier; a point at z = 0 gives one and does not fault.
 * Selection (iterate, :272-325) over the counts in hypothesis order, degenerate hypotheses skipped: `converged` is set
 * at the FIRST hypothesis with inliers > min_inliers and that one is selected; otherwise the selected one is the LAST
 * hypothesis whose count is >= every earlier one, from 0 (ties go to the later one, a count of 0 qualifies).  The
 * chunking into iterate(20) calls changes nothing (the members carry over); bNoMore is !converged.  N < min_inliers
 * (:257-261) is the caller's early exit: pass n_hyp = 0.
 * Three quirks of the reference are kept:
 *  (a) mvnMaxError1/2 are std::vector<size_t> (include/Sim3Solver.h:78-79), so 9.210 sigma2 (:129-130) is truncated
 *      to an integer before the float comparison: 9 at level 0, 13 at level 1.  max_err1/2 are compared as given; the
 *      caller passes floor(9.210 * (double)(float)sigma2).
 *  (b) A degenerate hypothesis returns at :399-400 before assigning anything, and CheckInliers rescores the previous
 *      hypothesis's transform: the previous count again, which can neither converge nor change the best values.  It is
 *      skipped, which is exact wherever the reference is defined (on the very first hypothesis it reads uninitialised
 *      members: skipped too), counted as 0 inliers and reported as LBA_S3R_DEGENERATE in hyp_flags.  Three exactly
 *      coincident points give N = 0, whose first unit vector (1, 0, 0, 0) is the eigenvector Eigen's maxCoeff and
 *      this solver both take: degenerate.
 *  (c) A hypothesis whose transform is not finite (a NaN scale from non-finite coordinates) scores 0 inliers,
 *      is reported as LBA_S3R_NONFINITE and can still be selected through 0 >= 0, as in the reference.
 * A batch is two launches: one wave per hypothesis, then one per pair; a pair's result does not depend on the batch or
 * on its position, and results are bitwise reproducible.
 * LBA_E_ARG: null tracker or arrays, n_cam < 1, a pair's correspondence, hypothesis or camera range
 * ([cam0, cam0 + 2 n_cam)) outside its array, cam1 / cam2 outside [0, n_cam), a triple with an index outside
 * [0, n_corr) of its pair or with a repeated index, min_inliers < 0, a max_err that is NaN.  LBA_E_LIMIT: n_cam > 64
 * (a pair's 2 n_cam camera records are kept in 16 KB of LDS), or a batch whose rows, hypotheses and inlier masks
 * (n_hyp * ceil(n_corr / 64) words per pair) exceed 2 GB; a pair's n_corr and n_hyp have no limit of their own.
 * A refused call writes nothing.  n_pairs == 0, n_corr == 0 and n_hyp == 0 for a pair (best_hyp = -1, every row
 * inlier = 0, q / t / s untouched) are valid.  When the correspondence ranges of two pairs overlap, the shared rows
 * carry the flags of the later pair.  hyp_S12 of a degenerate hypothesis is reported, not defined. */
#define LBA_S3R_DEGENERATE 1   /* hyp_flags: |vec| < 1e-5, the hypothesis was skipped */
#define LBA_S3R_NONFINITE  2   /* hyp_flags: q, t or s of the hypothesis is not finite */
typedef struct lba_s3r_corr {
    int32_t cam1, cam2;      /* mvncam1[i], mvncam2[i] (Sim3Solver.cc:93, :110-118) */
    int32_t inlier;          /* out: the selected hypothesis's mvbInliersi[i]; 0 when none is selected */
    int32_t pad;
    double  X1b[3], X2b[3];  /* mvX3Db1[i], mvX3Db2[i] (float, widened; :136-140) */
    double  max_err1, max_err2; /* mvnMaxError1/2[i] exactly as the reference holds them (quirk a) */
} lba_s3r_corr;
typedef struct lba_s3r_pair {
    double  q[4], t[3], s;   /* out: mBestRotation (as (x, y, z, w), w >= 0), mBestTranslation, mBestScale of the
                                selected hypothesis; untouched when best_hyp < 0 */
    int32_t fix_scale, min_inliers;   /* mbFixScale, mRansacMinInliers */
    int32_t corr0, n_corr, cam0;      /* cam0: its 2 n_cam lba_sim3_cam rows, KF1's then KF2's, as lba_sim3_optimize */
    int32_t hyp0, n_hyp;              /* its triples in `samples`: pair-local row indices */
    int32_t best_hyp, n_inliers, converged;   /* out: pair-local index or -1; its count or 0; bConverge */
} lba_s3r_pair;
int lba_sim3_ransac(lba_tracker* t, lba_s3r_pair* pairs, int32_t n_pairs, lba_s3r_corr* corr, int32_t n_corr,
                    const int32_t* samples, int32_t n_hyp,   /* [3 * n_hyp] */
                    const lba_sim3_cam* cams, int32_t n_cam_rows, int32_t n_cam,
                    double* hyp_S12 /* [8 n_hyp]: q t s */, int32_t* hyp_inliers, int32_t* hyp_flags); /* each may be NULL */
/* Measurement only: on != 0 makes lba_sim3_ransac bracket its two launches with two events on the tracker's stream;
 * last_ms (may be NULL) receives the kernel time of the last such call in milliseconds, or -1. */
int lba_sim3_ransac_profile(lba_tracker* t, int32_t on, double* last_ms);

/* ---- local mapping: the triangulation of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:408-587, with
 * GeometricTools::Triangulate, src/GeometricTools.cc:47-66, and MultiKeyFrame::UnprojectStereo, src/KeyFrame.cc:829-846)
 * for a batch of (keyframe, neighbour) pairs, the step that makes the landmarks the next lba_set_problem receives.  One
 * row is one match of SearchForTriangulation (lba_match_epipolar below: in this reference it decides every keypoint
 * on its own; Fuse stays on the CPU: greedy matching on map state); the
 * caller builds the rows (amc_lba.triangulate.tri_rows, :412-432, :498, :525, :565).  Per row, in fp64 on the
 * float-valued inputs widened, in the reference's order; the row gets the FIRST status that applies:
 *   rays      xn = ((u - cx) / fx, (v - cy) / fy, 1) of z1 / z2 with the row's camera (Pinhole::unprojectEig),
 *             ray = Rcw^T xn, cosRays their normalised dot product (:434-439).
 *   parallax  cosStereo1 = cosStereo2 = cosRays + 1; if side 1 is stereo (ur1 >= 0), cosStereo1 =
 *             cos(2 atan2(b1 / 2, depth1)); ONLY if side 1 is not stereo and side 2 is, cosStereo2 likewise (:441-450,
 *             quirk a); cosStereo = min of the two.  Evaluated as (d^2 - h^2) / (d^2 + h^2), h = b / 2, which is the same
 *             function of a finite depth (d = h = 0 gives 1, as atan2(0, 0) does); there is no transcendental.
 *   branch    triangulate when cosRays < cosStereo && cosRays > 0 && (stereo1 || stereo2 || cosRays < 0.9998); else
 *             back-project from KF1 when stereo1 && cosStereo1 < cosStereo2; else from KF2 when stereo2 &&
 *             cosStereo2 < cosStereo1; else LBA_TRI_PARALLAX (the final `else continue`, :461-481).
 *   Triangulate  A's rows x1 T1[2] - T1[0], y1 T1[2] - T1[1], x2 T2[2] - T2[0], y2 T2[2] - T2[1] (GeometricTools.cc:
 *             50-53); x3Dh the right singular vector of the smallest singular value (a one-sided Jacobi of 5 fixed
 *             sweeps on the columns of A; of equal singular values the first column's); w == 0 or w not finite is
 *             LBA_TRI_W_ZERO; X = x3Dh.head(3) / w, in which the vector's sign cancels.
 *   UnprojectStereo  z = depth; z <= 0 (or NaN) is LBA_TRI_NO_DEPTH; x = (k.u - cx) z invfx, y = (k.v - cy) z invfy
 *             with the RAW keypoint k and the LAST camera's cx, cy, invfx, invfy of that keyframe (cams[cam0 + n_cam -
 *             1]); X = Rwb (x, y, z) + twb: the BODY pose, not the camera's (quirk b).  stereo_point is set.
 *   gates     z1 = Tcw1[2] . (X, 1) <= 0: LBA_TRI_BEHIND1; z2 likewise: LBA_TRI_BEHIND2 (:489-495).  Reprojection in KF1
 *             then KF2 (:497-549): a mono side (ur < 0) drops e^2 > 5.991 sigma2 with u = fx x / z + cx; a stereo side
 *             drops ex^2 + ey^2 + er^2 > 7.8 sigma2 with invz = 1 / z, u = fx x invz + cx, u_r = u - bf invz, against z
 *             (the undistorted keypoint) and ur: LBA_TRI_REPROJ1 / LBA_TRI_REPROJ2.  dist = |X - Ow| of either camera;
 *             dist1 == 0 || dist2 == 0: LBA_TRI_DIST_ZERO (:558); far_points && (dist1 >= th_far || dist2 >= th_far):
 *             LBA_TRI_FAR (:561); ratioDist = dist2 / dist1, ratioOctave = scale1 / scale2, ratioDist ratio_factor <
 *             ratioOctave || ratioDist > ratioOctave ratio_factor: LBA_TRI_SCALE (:564-568).  Otherwise LBA_TRI_OK and X.
 * Quirks of the reference that are kept:
 *  (a) the `else if` of :448: with both sides stereo only cosStereo1 is computed, cosStereo2 stays cosRays + 1, so the
 *      back-projection can only come from KF1.
 *  (b) UnprojectStereo reads mvKeys (raw), the last camera's intrinsics and mRwb / mTwb, whatever camera the keypoint
 *      is in; tri_rows sets ur only for keypoints of the last camera, as :419-432 do.
 *  (c) every comparison is the reference's, so a NaN falls where it falls there: NaN <= 0 and NaN > gate are false, and
 *      a row with a NaN keypoint can come back LBA_TRI_OK with a NaN X, as the reference would create the point.
 *      Nothing loops on data.
 *  (d) LBA_TRI_DIST_ZERO cannot be reached with an Ow that is the camera's centre (z > 0 comes first); it stays because
 *      the device compares what it is given.
 * The reference computes all of this in float; the status of a row within float rounding of a gate can differ
 * (DESIGN.md §7 item 10 measures how often).
 * prm == NULL means ratio_factor = 1.5 * 1.2 and far_points = 0; the reference's is (double)(1.5f * mfScaleFactor)
 * (amc_lba.triangulate.ratio_factor).  n_new / n_stereo of a pair are `total` and `countStereo` (:572-574): its rows
 * with LBA_TRI_OK, and those of them with stereo_point.
 * A batch is one upload, one launch (one thread per row, one workgroup per 64 rows of a pair) and one download; a
 * row's result does not depend on the batch or on its position, and results are bitwise reproducible.
 * LBA_E_ARG: null tracker or arrays, a negative count, n_cam < 1, a pair's kf1 / kf2 outside [0, n_kf) or its rows
 * outside [0, n_rows), a keyframe's cameras [cam0, cam0 + n_cam) outside [0, n_cam_rows), cam1 / cam2 of a row of a
 * pair outside [0, n_cam), a ratio_factor that is not finite or not positive.  LBA_E_LIMIT: n_cam > 64 (a pair's
 * 2 n_cam camera records are kept in LDS), or an arena above 2 GB.  A refused call writes nothing.  n_pairs == 0 and a
 * pair with n_rows == 0 (n_new = n_stereo = 0) are valid.  Rows shared by two pairs carry the later pair's result. */
#define LBA_TRI_OK        0
#define LBA_TRI_PARALLAX  1    /* not enough parallax and no usable stereo depth */
#define LBA_TRI_W_ZERO    2    /* Triangulate returned false */
#define LBA_TRI_NO_DEPTH  3    /* UnprojectStereo found z <= 0 */
#define LBA_TRI_BEHIND1   4
#define LBA_TRI_BEHIND2   5
#define LBA_TRI_REPROJ1   6
#define LBA_TRI_REPROJ2   7
#define LBA_TRI_DIST_ZERO 8
#define LBA_TRI_FAR       9
#define LBA_TRI_SCALE     10
typedef struct lba_tri_cam {   /* one per (keyframe, camera) */
    double Tcw[12];            /* GetCameraPose(c).matrix3x4(), row-major, float widened (:360-361, :393-394) */
    double Ow[3];              /* GetCameraCenter(c) as the map holds it (:365, :398) */
    double fx, fy, cx, cy, invfx, invfy;   /* mvfx.. / minvfx.. of that camera, as held */
} lba_tri_cam;
typedef struct lba_tri_kf {
    double Rwb[9], twb[3];     /* mRwb (row-major), mTwb.translation(): what UnprojectStereo uses (KeyFrame.cc:841) */
    double bf, b;              /* mbf, mb */
    int32_t cam0, pad;         /* its n_cam rows of `cams` */
} lba_tri_kf;
typedef struct lba_tri_row {
    int32_t cam1, cam2;        /* mmpKeyToCam[idx1], [idx2] */
    int32_t status;            /* out: LBA_TRI_* */
    int32_t stereo_point;      /* out: bPointStereo */
    double  z1[2], z2[2];      /* mvKeysUn[idx].pt */
    double  k1[2], k2[2];      /* mvKeys[idx].pt: UnprojectStereo reads the raw keypoint (KeyFrame.cc:834-835) */
    double  ur1, ur2;          /* kp_ur: mvuRight[...] for the last camera, -1 otherwise (:419-432); bStereo = ur >= 0 */
    double  depth1, depth2;    /* mvDepth[mmpGlobalToLocalID[idx]] (read only when that side is stereo) */
    double  sigma2_1, sigma2_2;/* mvLevelSigma2[octave] */
    double  scale1, scale2;    /* mvScaleFactors[octave] */
    double  X[3];              /* out: x3D when status == LBA_TRI_OK, otherwise untouched */
} lba_tri_row;
typedef struct lba_tri_pair {
    int32_t kf1, kf2;          /* indices into `kfs`: mpCurrentKeyFrame, vpNeighKFs[i] */
    int32_t row0, n_rows;
    int32_t n_new, n_stereo;   /* out: `total` and `countStereo` of this pair */
} lba_tri_pair;
typedef struct lba_tri_params {
    double  ratio_factor, th_far;   /* 1.5f * mfScaleFactor; mThFarPoints */
    int32_t far_points, pad;        /* mbFarPoints */
} lba_tri_params;
int lba_triangulate(lba_tracker* t, lba_tri_pair* pairs, int32_t n_pairs, lba_tri_row* rows, int32_t n_rows,
                    const lba_tri_kf* kfs, int32_t n_kf, const lba_tri_cam* cams, int32_t n_cam_rows, int32_t n_cam,
                    const lba_tri_params* prm /* may be NULL */);
/* Measurement only: on != 0 makes lba_triangulate bracket its launch with two events on the tracker's stream;
 * last_ms (may be NULL) receives the kernel time of the last such call in milliseconds, or -1. */
int lba_triangulate_profile(lba_tracker* t, int32_t on, double* last_ms);

/* ---- local mapping: ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:947-1131, with Pinhole::project and
 * Pinhole::epipolarConstrain, src/CameraModels/Pinhole.cpp:43-49, 107-129) for a batch of (keyframe, neighbour) pairs:
 * the matcher whose vMatchedPairs are the rows of lba_triangulate.  It reuses lba_tri_kf / lba_tri_cam as they are
 * (Tcw, Ow, fx, fy, cx, cy, cam0), so a caller builds those arrays once for both calls.
 * The function is NOT greedy in this reference: vbMatched2 is declared (:979) and read (:1028) but never set, the map
 * is read as it is on entry and nothing is written to it, so every keypoint of KF1 is decided on its own.
 *   tables    per (pair, c1, c2): T12 = T1cw(c1) T2cw(c2)^-1, i.e. R12 = R1 R2^T, t12 = R1 Ow2 + t1;
 *             F12 = ((K1^-T [t12]x) R12) K2^-1; the epipole ep = project2(R2 Ow1 + t2) = (fx x / z + cx, fy y / z + cy)
 *             with no test on z.
 *   walk      the nodes present in BOTH keyframes' feature vectors, in ascending node id (the merge with lower_bound).
 *   idx1      every entry of KF1's list of a common node: has_point -> LBA_EPI_HAS_POINT; only_stereo and not stereo ->
 *             LBA_EPI_NOT_STEREO.  Stereo is cam == n_cam - 1 && u_right >= 0 (`>= 0`: lba_match_project's rule is > 0).
 *   idx2      every entry of KF2's list of that node IN LIST ORDER, from bestDist = th_low, bestIdx2 = -1: skipped when
 *             it has a point, or under only_stereo is not stereo; dist = the 256-bit Hamming distance, skipped when
 *             dist > th_low || dist > bestDist; when neither side is stereo, skipped when
 *             (ep.x - x2)^2 + (ep.y - y2)^2 < 100 scale2 (KF2's scale of the candidate); unless `coarse` the epipolar
 *             gate: (a, b, c) = (x1, y1, 1) F12, num = a x2 + b y2 + c, den = a^2 + b^2, den == 0 fails, else it passes
 *             when num^2 / den < 3.84 unc with unc = sigma2 of the CANDIDATE (KF2).  A candidate that passes becomes
 *             bestIdx2 with bestDist = dist.
 *   result    bestIdx2 >= 0: LBA_EPI_OK; else LBA_EPI_NO_MATCH.  A keypoint of KF1 that is in no node, or whose node
 *             KF2 does not hold: LBA_EPI_NO_NODE.  n_matches of a pair is the reference's nmatches; its rows with
 *             LBA_EPI_OK in ascending idx1 are vMatchedPairs (amc_lba.epipolar.epi_matches).
 *   check_orientation (CreateNewMapPoints builds ORBmatcher(0.6f, false): off): the histogram of :1071-1081 and
 *             ComputeThreeMaxima on the host after the download; quirk (c).
 * Precision: the tracker's convention, like lba_triangulate: fp64 on the float-valued inputs
 * widened, in the reference's order; results are held against the restatement on SETTLED jobs only (every comparison
 * further than 1e-9 relative from its gate).  NOT lba_match_project's float-bit convention: F12 goes through Eigen's
 * float 3 x 3 inverse and three matrix products, whose operation order nobody can reproduce.
 * Quirks of the reference that are kept:
 *  (a) vbMatched2 is never set: several idx1 may get the same idx2; no state passes between keypoints.
 *  (b) ties go to the LAST candidate in node-list order that passes the gates (`dist > bestDist` is the skip); a
 *      candidate at distance exactly th_low can win; with bestDist shrinking a later candidate is tested only if
 *      dist <= bestDist.
 *  (c) the rotation pass removes the matches of the bins that ARE ind1, ind2 or ind3 (:1108 reads `i == ind1 || ...`,
 *      the opposite of the projection search); n_matches loses one each; the row becomes LBA_EPI_ROT, idx2 is kept.
 *  (d) unc is KF2's level sigma2 (kp1's sigmaLevel is passed and never read); 3.84 * unc is a double product there and
 *      here.
 *  (e) an epipole with z <= 0 falls where IEEE puts it: negative depth mirrors it, z == 0 gives +-inf or NaN, every
 *      comparison with those is false, so nothing is skipped by the epipole test.
 *  (f) den == 0 is false: two cameras with the same centre give t12 = 0, F12 = 0 and no match unless `coarse`.
 *  (g) a node that only one keyframe holds contributes nothing.
 * A batch is one upload, two launches (k_epi_tables: one thread per (pair, c1, c2); k_epi_match: one 64-lane wave per
 * (pair, common node, chunk of 64 entries of KF1's list), the lane IS the idx1 and walks KF2's list in order) and one
 * download; a keyframe's features and node lists are uploaded once however many pairs name it.  A pair's result does
 * not depend on the batch and is bitwise reproducible.
 * LBA_E_ARG: null tracker or arrays, a negative count, n_cam < 1, a range outside its array, a keyframe's cameras
 * outside `cams`, node_id not strictly ascending within a keyframe, node_start not starting at 0, decreasing or past
 * the end of node_feat, a node_feat entry outside [0, n_feat) or listed twice in one keyframe, a feature's cam outside
 * [0, n_cam), th_low outside [0, 255], a pair's kf1 / kf2 outside [0, n_kf), two pairs whose `out` ranges overlap or a
 * range that does not fit in [0, n_out).  LBA_E_LIMIT: n_cam > 64, or an arena above 2 GB.  A refused call writes
 * nothing and sets lba_tracker_last_error.  n_pairs == 0, a keyframe without features or without nodes and a pair
 * with kf1 == kf2 are valid. */
#define LBA_EPI_OK         0
#define LBA_EPI_HAS_POINT  1
#define LBA_EPI_NOT_STEREO 2
#define LBA_EPI_NO_NODE    3    /* the keypoint is in no node, or its node is not in KF2 */
#define LBA_EPI_NO_MATCH   4    /* no candidate passed */
#define LBA_EPI_ROT        5    /* accepted, then removed by quirk (c); idx2 is kept */
typedef struct lba_epi_feat {      /* 64 bytes, one per keypoint of a keyframe, in the keyframe's global keypoint order */
    float    x, y;                 /* mvKeysUn[idx].pt */
    float    angle;                /* mvKeysUn[idx].angle (read with check_orientation only) */
    float    u_right;              /* mvuRight[mmpGlobalToLocalID[idx]], anything < 0 where there is none */
    float    scale;                /* mvScaleFactors[octave] */
    float    sigma2;               /* mvLevelSigma2[octave] */
    int32_t  cam;                  /* mmpKeyToCam[idx] */
    int32_t  has_point;            /* GetMapPoint(idx) != NULL on entry */
    uint32_t desc[8];
} lba_epi_feat;
typedef struct lba_epi_kf {        /* parallel to kfs[]: entry k describes lba_tri_kf k */
    int32_t feat0, n_feat;         /* its rows of `feats` */
    int32_t node0, n_node;         /* mFeatVec, node ids strictly ascending: its n_node rows of node_id and its n_node + 1
                                      rows of node_start, both from row node0 (a packer gives a keyframe n_node + 1 rows) */
    int32_t nf0, pad;              /* its entries of node_feat; node_start holds n_node + 1 offsets from nf0, the first 0 */
} lba_epi_kf;
typedef struct lba_epi_pair {
    int32_t kf1, kf2;
    int32_t out0;                  /* its n_feat(kf1) rows of `out` */
    int32_t n_matches;             /* out */
} lba_epi_pair;
typedef struct lba_epi_row {       /* out, one per (pair, keypoint of KF1) */
    int32_t idx2;                  /* bestIdx2 (keyframe-local keypoint index of KF2), or -1 */
    int32_t dist;                  /* bestDist of the accepted candidate; th_low where idx2 == -1 */
    int32_t status;                /* LBA_EPI_* */
    int32_t pad;
} lba_epi_row;
typedef struct lba_epi_params { int32_t th_low, only_stereo, coarse, check_orientation; } lba_epi_params;  /* NULL: 50,0,0,0 */
int lba_match_epipolar(lba_tracker* t, lba_epi_pair* pairs, int32_t n_pairs, lba_epi_row* out, int32_t n_out,
                       const lba_tri_kf* kfs, const lba_epi_kf* ekfs, int32_t n_kf,
                       const lba_tri_cam* cams, int32_t n_cam_rows, int32_t n_cam,
                       const lba_epi_feat* feats, int32_t n_feats, const int32_t* node_id, const int32_t* node_start,
                       int32_t n_node_rows, const int32_t* node_feat, int32_t n_node_feat, const lba_epi_params* prm);
/* Measurement only: on != 0 makes lba_match_epipolar bracket its two launches with events on the tracker's stream;
 * last_ms (may be NULL) receives the two kernel times (k_epi_tables, k_epi_match) of the last such call, or -1. */
int lba_match_epipolar_profile(lba_tracker* t, int32_t on, double* last_ms);

/* ---- loop closing and relocalisation: ORBmatcher::SearchByBoW for a batch of pairs, both overloads:
 *   LBA_BOW_KF     (pKF1, pKF2, vpMatches12), src/ORBmatcher.cc:805-945: LoopClosing::DetectCommonRegionsFromBoW calls
 *                  it once per (candidate, covisible keyframe) with mpCurrentKF as KF1 (LoopClosing.cc:485-496), the
 *                  stage in front of lba_sim3_ransac and lba_sim3_optimize;
 *   LBA_BOW_FRAME  (pKF, F, vpMapPointMatches), :227-421: Tracking::TrackReferenceKeyFrame.  Side 1 is the keyframe,
 *                  side 2 the frame.
 * `ekfs`, `feats`, `node_id`, `node_start` and `node_feat` are exactly lba_match_epipolar's arrays (a frame is one more
 * lba_epi_kf entry); there are no keyframe poses and no cameras, the matcher has no geometry: of lba_epi_feat only
 * desc, has_point and (with check_orientation) angle are read.  has_point means "has a map point that is not bad"
 * (:844-848, :864-870); has_point of side 2 is ignored in LBA_BOW_FRAME.  `angle` is whatever the caller's overload
 * reads: mvKeysUn[..].angle on both sides at :897, but F.mvKeys[bestIdxF].angle, the RAW keypoint, for the frame at
 * :342.
 *   walk      the nodes present in BOTH sides' feature vectors, in ascending node id (the merge with lower_bound).
 *   idx1      every entry of side 1's list of a common node IN LIST ORDER: without has_point -> LBA_BOW_NO_POINT.
 *   idx2      every entry of side 2's list of that node in list order, from bestDist1 = bestDist2 = 256, bestIdx2 = -1:
 *             skipped when it is matched already (vbMatched2[idx2], or vpMapPointMatches[idx2] != NULL: set by an
 *             EARLIER idx1 of this call) or, in LBA_BOW_KF, has no point; dist = the 256-bit Hamming distance;
 *             dist < bestDist1: bestDist2 = bestDist1, bestDist1 = dist, bestIdx2 = idx2; else dist < bestDist2:
 *             bestDist2 = dist.
 *   accept    bestDist1 < th_low (LBA_BOW_KF) or bestDist1 <= th_low (LBA_BOW_FRAME), else LBA_BOW_NO_CAND; then
 *             (float)bestDist1 < nn_ratio * (float)bestDist2 (one float product), else LBA_BOW_RATIO; accepted:
 *             LBA_BOW_OK and idx2 is matched from here on.
 *   rotation  with check_orientation, on the host after the download: the ORDINARY rule (:932-941, :408-417): the
 *             matches of the bins that are NOT one of ComputeThreeMaxima's three are removed (LBA_BOW_ROT, idx2 kept).
 *             This is the opposite of lba_match_epipolar's quirk (c).  A removed match stays matched for the scan: the
 *             pass runs after the loops.
 *   result    idx2, dist, dist2 of a row are bestIdx2, bestDist1, bestDist2 as the reference holds them after the inner
 *             loop, for every status that ran it (OK, NO_CAND, RATIO, ROT); -1, 256, 256 for NO_POINT and NO_NODE.
 *             n_matches of a pair is the reference's return value.  The output is indexed by the keypoint of side 1 in
 *             both modes: vpMatches12[idx1] = the point of row.idx2 (LBA_BOW_KF); a LBA_BOW_FRAME caller scatters
 *             vpMapPointMatches[row.idx2] = the point of idx1 (amc_lba.bow.frame_matches).  idx2 is unique among the
 *             OK and ROT rows of a pair.
 * The matched flag is indexed by idx2 and DBoW2 puts every feature into exactly one node (TemplatedVocabulary::transform
 * calls addFeature once per feature), so no state crosses a node: every (pair, common node) is an independent, short
 * sequential problem.  k_bow_match gives one 64-lane wave to each: idx1 serially, the node's candidates in parallel
 * (lane l owns l, l + 64, ...; its matched flags are 32 bits of a register), the best and the second best by one
 * wave-wide merge of the lanes' scans (lba_bow_math.hpp has the proof that a scan may be split).  The results are the reference's own,
 * bit for bit; a pair's result does not depend on the batch.  One upload, one launch, one download; a keyframe's
 * features and node lists go up once however many pairs name it.
 * LBA_E_ARG: null tracker or arrays, a negative count, a range outside its array, node_id not strictly ascending
 * within a keyframe, node_start not starting at 0, decreasing or past the end of node_feat, a node_feat entry outside
 * [0, n_feat) or listed twice in one keyframe (what makes nodes independent), a pair's kf1 / kf2 outside [0, n_kf),
 * two pairs whose `out` ranges overlap or a range that does not fit in [0, n_out), th_low outside [0, 255], nn_ratio
 * not finite, an unknown mode.  LBA_E_LIMIT: a side-2 node list longer than LBA_BOW_MAX_NODE, or an arena above 2 GB.
 * A refused call writes nothing and sets lba_tracker_last_error.  n_pairs == 0, a keyframe without features or without
 * nodes and a pair with kf1 == kf2 are valid. */
#define LBA_BOW_KF    0   /* :805  side 2 needs a point; accept bestDist1 <  th_low */
#define LBA_BOW_FRAME 1   /* :227  side 2 = frame features, no point needed; accept bestDist1 <= th_low */
#define LBA_BOW_OK       0
#define LBA_BOW_NO_POINT 1    /* idx1 has no usable point */
#define LBA_BOW_NO_NODE  2    /* the keypoint is in no node, or its node is not in side 2 */
#define LBA_BOW_NO_CAND  3    /* the threshold failed; this includes an empty list */
#define LBA_BOW_RATIO    4    /* the ratio test failed */
#define LBA_BOW_ROT      5    /* accepted, then removed by the rotation pass; idx2 is kept and stays matched */
#define LBA_BOW_MAX_NODE 2048 /* entries of one node's list on side 2 */
typedef struct lba_bow_pair { int32_t kf1, kf2, out0, n_matches /* out */; } lba_bow_pair;
typedef struct lba_bow_row  { int32_t idx2, dist, dist2, status; } lba_bow_row;   /* one per (pair, keypoint of side 1) */
typedef struct lba_bow_params { int32_t mode, th_low; float nn_ratio; int32_t check_orientation; } lba_bow_params;
/* prm NULL: LBA_BOW_KF, 50, 0.9f, 1 (LoopClosing's matcherBoW(0.9, true)) */
int lba_match_bow(lba_tracker* t, lba_bow_pair* pairs, int32_t n_pairs, lba_bow_row* out, int32_t n_out,
                  const lba_epi_kf* ekfs, int32_t n_kf, const lba_epi_feat* feats, int32_t n_feats,
                  const int32_t* node_id, const int32_t* node_start, int32_t n_node_rows,
                  const int32_t* node_feat, int32_t n_node_feat, const lba_bow_params* prm);
/* Measurement only: on != 0 makes lba_match_bow bracket its launch with two events on the tracker's stream;
 * last_ms (may be NULL) receives the kernel time of the last such call in milliseconds, or -1. */
int lba_match_bow_profile(lba_tracker* t, int32_t on, double* last_ms);

/* ---- tracking: ORBmatcher's two projection searches for a batch of frames: SearchByProjection(MultiFrame&,
 * const vector<MapPoint*>&, th, ...) (src/ORBmatcher.cc:43-217, Tracking::SearchLocalPoints) is LBA_MATCH_RATIO, and
 * SearchByProjection(MultiFrame& Current, const MultiFrame& Last, th, bMono) (:1439-1568, TrackWithMotionModel) is
 * LBA_MATCH_BEST.  A *search* is one frame with its ordered job list; a *job* is one (map point, camera) pair the
 * reference's loops reach, in their order (point-major, cameras inner).  The caller projects (isInFrustum's fields, or
 * uv / invzc / the octave: amc_lba.match.jobs_local_points / jobs_last_frame) and passes the results as floats:
 * reproducing Eigen's float SE3f * Vector3f bit for bit is not a goal of this entry point.
 *
 * Per job, MultiFrame::GetFeaturesInArea (src/Frame.cc:608-673) on the caller's grid (a CSR of the 64 x 48 cells per
 * camera, cells in [ix][iy] order, a cell's features in AssignFeaturesToGrid's insertion order): the cell rectangle
 *   max(0, (int)floor((x - min_x - radius) * grid_w_inv)) .. min(63, (int)ceil((x - min_x + radius) * grid_w_inv))
 * and its y sibling, the level test, fabs(kx - x) < radius && fabs(ky - y) < radius; then, per candidate in
 * (ix, iy, position in cell) order: skip a taken feature, the stereo gate (u_right > 0 and fabs(ur - u_right) >
 * radius skips), the 256-bit Hamming distance, best (LBA_MATCH_BEST) or best and second best with their levels
 * (LBA_MATCH_RATIO), `dist < bestDist` strict.  Accepted (LBA_MATCH_OK): bestDist <= th_high, and in LBA_MATCH_RATIO
 * not (bestLevel == bestLevel2 && bestDist > nn_ratio * bestDist2).  An accepted job writes its point to its best
 * feature, and if `blocks` (the point's Observations() > 0) that feature is taken for every later job.
 * Every floating-point expression that decides something is evaluated in FLOAT, in the reference's order, without
 * contraction (a stated departure from the tracker's fp64-on-widened-inputs convention): each is
 * one to three IEEE single operations, so the decisions are the reference's own bits and all outputs are exact.
 * With check_orientation (LBA_MATCH_BEST only) the rotation histogram of :1526-1567 with ComputeThreeMaxima follows:
 * rot = job.angle - feat.angle, +360 if negative, bin = round(rot * (1.0f / 30)), 30 -> 0; the jobs of every bin that is
 * not one of the (up to) three maxima become LBA_MATCH_ROT, their features' `job` -1, and n_matches loses one each.
 * Quirks of the reference that are kept:
 *  (a) bCheckLevels = (min_level > 0) || (max_level >= 0): a min_level of 0 or -1 with max_level < 0 checks nothing;
 *      octave < min_level is applied even where max_level < 0.
 *  (b) the last-frame function truncates: `int uRight = mvuRight[..]` before `uRight > 0` and before the subtraction
 *      (:1500-1503); the local-points function compares the float (:95-98).  params.ur_truncate selects.
 *  (c) the window's high side uses ceil, so it reaches one cell further than floor; PosInGrid rounds.  The caller's CSR
 *      is the reference's grid, so both stay.
 *  (d) ties go to the first candidate in (ix, iy, position in cell) order; a single candidate is accepted in
 *      LBA_MATCH_RATIO (bestLevel2 stays -1); a candidate at distance 256 is never chosen (256 < 256 is false).
 *  (e) x, y or radius not finite, or a floor / ceil value outside int's range, is undefined behaviour there
 *      ((int)floor(NaN)); here such a job has no candidates (LBA_MATCH_NO_CAND).  The values are clamped in float
 *      before the conversion; for every finite in-range value the result is the reference's.
 *  (f) the rotation pass clears mvpMapPoints[feature] for EVERY entry of a losing bin: a feature that a non-blocking
 *      job of a losing bin won and a later job of a surviving bin overwrote ends with `job` -1 although the later job
 *      stays LBA_MATCH_OK.  n_matches_mono is not reduced by the rotation pass (the reference's nmatches_mono is not).
 * n_matches counts accepted jobs including overwrites; n_matches_mono those with cam < n_cam - 1.
 *
 * Device: k_match_gather, one 64-lane wave per job, writes each job's candidates (gates applied, `taken` not) in
 * order; k_match_resolve, one workgroup per (search, camera), reproduces the sequential loop exactly in rounds (a job is
 * final once no earlier pending job of its camera shares an untaken candidate with it); cam.rounds reports the count,
 * at most the camera's job count, 0 for a camera without jobs.  One upload, two launches, one download; nothing waits
 * on another workgroup.  The rotation pass and the counts run on the host after the download.
 * LBA_E_ARG: null tracker or arrays; a negative count; a search's camera, feature, job, cell_start or cell_feat range
 * outside its array, or its cameras, features or jobs beginning before the end of the search before (the searches lie
 * one behind the other); n_cam < 1; cell_start not starting at 0 or decreasing, or past n_cell_feat; a cell_feat entry
 * outside [0, n_feat) or naming a feature of another camera than the cell's; a feature's cam outside [0, n_cam) or its
 * octave outside [0, 255]; a job's cam outside [0, n_cam) or min_level > max_level where max_level >= 0; mode not
 * one of the two; th_high outside [0, 255]; nn_ratio NaN; stereo_cam outside [-1, n_cam) of any search;
 * check_orientation with LBA_MATCH_RATIO.  LBA_E_LIMIT: more than LBA_MATCH_MAX_FEAT features in one camera (the
 * resolve kernel keeps a word and a bit per feature in LDS), or an arena above 2 GB.  A refused call writes nothing
 * and sets the text lba_tracker_last_error returns.  n_searches == 0, a search without jobs or without features
 * are valid. */
#define LBA_MATCH_RATIO 0
#define LBA_MATCH_BEST  1
#define LBA_MATCH_OK       0
#define LBA_MATCH_NO_CAND  1   /* vIndices empty, or every candidate skipped (taken / stereo gate) */
#define LBA_MATCH_TOO_FAR  2   /* bestDist > th_high */
#define LBA_MATCH_RATIO_FAIL 3 /* LBA_MATCH_RATIO: equal levels and bestDist > nn_ratio * bestDist2 */
#define LBA_MATCH_ROT      4   /* accepted, then removed by the rotation check */
#define LBA_MATCH_MAX_FEAT 8192
#define LBA_MATCH_GRID_COLS 64
#define LBA_MATCH_GRID_ROWS 48
typedef struct lba_match_cam {     /* one per (search, camera) */
    float   min_x, min_y;          /* mvMinX[c], mvMinY[c] */
    float   grid_w_inv, grid_h_inv;/* mvGridElementWidthInv[c], mvGridElementHeightInv[c] */
    int32_t rounds;                /* out: rounds k_match_resolve needed for this camera's jobs */
} lba_match_cam;
typedef struct lba_match_feat {    /* 64 bytes */
    float    x, y;                 /* mvKeysUn[idx].pt */
    float    angle;                /* mvKeysUn[idx].angle */
    float    u_right;              /* mvuRight[mmpGlobalToLocalID[idx]]; <= 0: none */
    int32_t  octave;               /* mvKeysUn[idx].octave, 0 .. 255 */
    int32_t  cam;                  /* mmpKeyToCam[idx] */
    int32_t  taken;                /* in: mvpMapPoints[idx] holds a point with Observations() > 0 on entry */
    int32_t  job;                  /* out: search-local index of the job whose point it holds at the end, or -1 */
    uint32_t desc[8];
} lba_match_feat;
typedef struct lba_match_job {     /* 96 bytes */
    float    x, y;                 /* mvTrackProjX / Y[c], or uv */
    float    radius;               /* r * mvScaleFactors[level] (the float product), or th * mvScaleFactors[octave] */
    float    ur;                   /* mvTrackProjXR[c], or uv(0) - mbf * invzc */
    float    angle;                /* LBA_MATCH_BEST with check_orientation: LastFrame.mvKeysUn[i].angle */
    int32_t  cam;
    int32_t  min_level, max_level;
    int32_t  point;                /* opaque, echoed */
    int32_t  blocks;               /* the point's Observations() > 0 */
    uint32_t desc[8];              /* pMP->GetDescriptor() */
    int32_t  feat;                 /* out: search-local feature won (kept under LBA_MATCH_ROT), or -1 */
    int32_t  status;               /* out: LBA_MATCH_* */
    int32_t  best_dist, best_dist2;/* out: bestDist, bestDist2 (256: none; best_dist2 is 256 in LBA_MATCH_BEST) */
    int32_t  pad[2];
} lba_match_job;
typedef struct lba_match_search {
    int32_t cam0, n_cam;           /* its rows of `cams` */
    int32_t feat0, n_feat;         /* its rows of `feats`; cell_feat and the outputs number them from 0 */
    int32_t job0, n_jobs;          /* its rows of `jobs`, in the reference's loop order */
    int32_t cell0;                 /* its n_cam * 64 * 48 + 1 entries of `cell_start` (offsets from cf0, the first 0) */
    int32_t cf0;                   /* its entries of `cell_feat` */
    int32_t n_matches, n_matches_mono;   /* out */
} lba_match_search;
typedef struct lba_match_params {
    int32_t mode;                  /* LBA_MATCH_RATIO / LBA_MATCH_BEST */
    int32_t th_high;               /* TH_HIGH (100) */
    float   nn_ratio;              /* mfNNratio */
    int32_t stereo_cam;            /* camera whose features pass the u_right gate (the reference: n_cam - 1); -1 none */
    int32_t ur_truncate;           /* quirk (b) */
    int32_t check_orientation;     /* mbCheckOrientation; LBA_MATCH_BEST only */
} lba_match_params;
int lba_match_project(lba_tracker* t, lba_match_search* searches, int32_t n_searches, lba_match_cam* cams,
                      int32_t n_cams, const int32_t* cell_start, int32_t n_cell_start, const int32_t* cell_feat,
                      int32_t n_cell_feat, lba_match_feat* feats, int32_t n_feats, lba_match_job* jobs, int32_t n_jobs,
                      const lba_match_params* prm);
/* Measurement only: on != 0 makes lba_match_project bracket its two launches with events on the tracker's stream;
 * last_ms (may be NULL) receives {k_match_gather, k_match_resolve} of the last such call in milliseconds, or -1. */
int lba_match_profile(lba_tracker* t, int32_t on, double* last_ms /* [2] */);
/* The text of the last refusal or failure of a call on this tracker ("" before the first). */
const char* lba_tracker_last_error(const lba_tracker* t);

/* ---- loop closing: the Sim3 ORBmatcher::SearchByProjection, both overloads (src/ORBmatcher.cc:423-548 and :550-685;
 * LoopClosing.cc:586, :608 and :800), for a batch of hypotheses against ONE keyframe.  The keyframe (its features, its
 * 64 x 48 CSR grid as one search of lba_match_project has it, one lba_match_cam and one lba_s3p_cam per camera) is shared
 * by the whole batch; every *search* is a hypothesis: its own Sbw and its own range of `points`.  A *job* is one
 * (search, point, camera), in the reference's loop order (point-major, cameras inner): row `row0 + p * n_cam + c`.
 *
 * Per (search, camera), in fp64 on the float inputs widened (the tracker's convention): Tbw = (R(Sbw), t / s),
 * Twb = Tbw^-1, Tcl = Tbw_kf * Tbw_prev^-1, Twl = Twb * Tcl, Twb_c = QueryPose(Twl, Twb, v_prev, v, stamp_prev, stamp,
 * stamp_c), Tcw[c] = (Twb_c * Tbc[c])^-1, written as 12 doubles (R row-major, then t) and rounded ONCE to 12 floats.  The
 * reference rounds Twb_c to float and finishes in SE3f; its float quaternion products are not reproduced (as for
 * lba_match_project).  QueryPose does not depend on Qc, so none is passed.
 * Per job, in FLOAT, in this operation order, without contraction, divide and square root correctly rounded:
 *   p3Dc = ((r0 x + r1 y) + r2 z) + t per row; z < 0 -> BEHIND;
 *   proj_form 0 (Pinhole::project, :480): u = fx * X / Z + cx; proj_form 1 (:610-615): invz = 1 / Z, u = fx * (X * invz) + cx;
 *   IsInImage: u >= min_x && u < max_x && v >= min_y && v < max_y, else OUT_OF_IMAGE;
 *   PO = p - ow[c], dist = sqrt((x^2 + y^2) + z^2); dist < min_dist || dist > max_dist -> DIST;
 *   (PO.x n.x + PO.y n.y) + PO.z n.z < 0.5f * dist -> ANGLE;
 *   PredictScale: ratio = max_distance / dist in float, level = ceil(log((double)ratio) / (double)log_scale_factor),
 *   clamped to [0, n_levels - 1]; radius = (float)th * scale_factors[level];
 *   GetFeaturesInArea's rectangle and window test, keypoint levels [level - 1, level], the Hamming distance, the best with
 *   strict <, the first on a tie, 256 never wins; accepted when (float)best_dist <= (float)th_low * ratio_hamming; an
 *   accepted job takes its feature for every later job of the search (vpMatched[bestIdx] = pMP).
 * Quirks of the reference that are kept:
 *  (a) PO and dist use GetCameraCenter(c) of the MAP pose (ow), the projection uses the Sim3-corrected pose (:489, :624).
 *  (b) a point that matched in camera c goes on to camera c + 1 and may match again; n_matches counts both.
 *  (c) spAlreadyFound is built once on entry: `skip` is the caller's isBad() || spAlreadyFound.count(pMP).
 *  (d) z == 0 passes `z < 0.0`; the projection is +-inf or NaN, every IsInImage comparison fails: OUT_OF_IMAGE.
 *  (e) Ow = Tbw^-1's translation is computed there and never read; it is not computed here.
 *  (f) `0.5 * dist` is a double product there; halving is exact, so 0.5f * dist decides the same.
 *  (g) with floor(th_low * ratio_hamming) >= 256 the reference indexes vpMatched[-1]: refused with LBA_E_ARG.
 *  (h) dist == 0 or a ratio that is not finite makes (int)ceil(..) undefined there.  Here the quotient is clamped before
 *      the conversion: NaN -> level 0, +inf -> n_levels - 1, -inf -> 0.
 * Device (lba_sim3_project.hip): k_s3p_pose, k_s3p_project (one thread per job), k_s3p_compact (one workgroup per
 * (search, camera): its live jobs in order and their list offsets), k_s3p_base, ONE readback of the per-(search, camera)
 * totals that sizes the candidate lists, k_s3p_gather (one wave per live job), k_s3p_resolve (one workgroup per (search,
 * camera): the sequential loop exactly, in rounds, as k_match_resolve).  One upload, one download; nothing waits on
 * another workgroup.  A search's result does not depend on the batch or on its position.
 * LBA_E_ARG: null tracker or arrays, a negative count, n_cam < 1, n_levels < 1, a malformed grid (as lba_match_project), a
 * search's point range outside `points`, its taken row outside `taken`, its rows, feature entries or poses outside their
 * arrays or beginning before the end of the search before, th < 0, th_low < 0, a ratio_hamming that is not finite or
 * negative, quirk (g), a proj_form other than 0 or 1.  LBA_E_LIMIT: n_cam > 64, more than LBA_MATCH_MAX_FEAT features in
 * one camera, arena and candidate lists above 2 GB.  A refused call writes nothing and sets lba_tracker_last_error.
 * n_searches == 0, a search without points, a keyframe without features and has_prev == 0 (every row LBA_S3P_NO_PREV,
 * n_matches 0, as the reference returns before it projects) are valid. */
#define LBA_S3P_OK           0
#define LBA_S3P_NO_CAND      1   /* no candidate in the window, or every one taken or at another level */
#define LBA_S3P_TOO_FAR      2   /* bestDist > TH_LOW * ratioHamming */
#define LBA_S3P_SKIPPED      3
#define LBA_S3P_BEHIND       4
#define LBA_S3P_OUT_OF_IMAGE 5
#define LBA_S3P_DIST         6
#define LBA_S3P_ANGLE        7
#define LBA_S3P_NO_PREV      8
#define LBA_S3P_MAX_CAM      64
typedef struct lba_s3p_kf {        /* 136 bytes */
    double  stamp, stamp_prev;     /* mTimeStamp of the keyframe and of mPrevKF */
    float   q[4], t[3];            /* GetPose(): q as x, y, z, w */
    float   q_prev[4], t_prev[3];  /* mPrevKF->GetPose() */
    float   v[6], v_prev[6];       /* GetVelocity() of both */
    float   log_scale_factor;      /* mfLogScaleFactor */
    int32_t has_prev;              /* mPrevKF != NULL */
    int32_t n_levels;              /* mnScaleLevels: entries of scale_factors */
    int32_t n_cam;
} lba_s3p_kf;
typedef struct lba_s3p_cam {       /* 88 bytes */
    double  stamp;                 /* mvTimeStamps[c] */
    float   q_bc[4], t_bc[3];      /* mTbc[c] */
    float   fx, fy, cx, cy;
    float   min_x, max_x, min_y, max_y;   /* mvMinX[c] .. mvMaxY[c] */
    float   ow[3];                 /* GetCameraCenter(c) of the map pose: quirk (a) */
    int32_t pad[2];
} lba_s3p_cam;
typedef struct lba_s3p_point {     /* 80 bytes */
    float    pos[3], normal[3];    /* GetWorldPos(), GetNormal() */
    float    min_dist, max_dist;   /* GetMinDistanceInvariance(), GetMaxDistanceInvariance() (with 0.8 / 1.2) */
    float    max_distance;         /* mfMaxDistance, raw: PredictScale reads it */
    int32_t  skip;                 /* isBad() || spAlreadyFound.count(pMP) */
    uint32_t desc[8];
    int32_t  pad[2];
} lba_s3p_point;
typedef struct lba_s3p_search {    /* 64 bytes */
    float   q[4], t[3], s;         /* Sbw */
    int32_t point0, n_points;      /* its range of `points` (ranges may be shared) */
    int32_t taken0;                /* its n_feats bytes of `taken` (vpMatched[idx] != NULL on entry), or -1: all free */
    int32_t row0;                  /* its n_points * n_cam rows of `rows` */
    int32_t featpt0;               /* its n_feats entries of `feat_point` */
    int32_t pose0;                 /* its n_cam entries of `poses` */
    int32_t n_matches;             /* out */
    int32_t pad;
} lba_s3p_search;
typedef struct lba_s3p_row {       /* out, 32 bytes: one job */
    int32_t status;                /* LBA_S3P_* */
    int32_t feat;                  /* the feature won, or -1 */
    int32_t best_dist;             /* 256: none */
    int32_t level;                 /* nPredictedLevel, -1 for a job that failed a gate */
    float   x, y, radius;          /* echoed; 0 where they were not reached */
    int32_t pad;
} lba_s3p_row;
typedef struct lba_s3p_pose {      /* out, 152 bytes: one (search, camera) */
    double  tcw_d[12];             /* Tcw[c] before rounding: R row-major, t */
    float   tcw[12];               /* what the jobs use */
    int32_t rounds;                /* rounds k_s3p_resolve needed */
    int32_t pad;
} lba_s3p_pose;
typedef struct lba_s3p_params {
    int32_t th, th_low;            /* th; TH_LOW (50) */
    float   ratio_hamming;
    int32_t proj_form;             /* 0: fx * X / Z + cx (:480); 1: fx * (X * (1 / Z)) + cx (:610-615) */
} lba_s3p_params;
/* feat_point[featpt0 + f]: the search-local index of the point feature f holds at the end (vpMatched), or -1. */
int lba_match_sim3_project(lba_tracker* t, const lba_s3p_kf* kf, const lba_s3p_cam* kcams, const lba_match_cam* gcams,
                           const float* scale_factors, const int32_t* cell_start, int32_t n_cell_start,
                           const int32_t* cell_feat, int32_t n_cell_feat, const lba_match_feat* feats, int32_t n_feats,
                           lba_s3p_search* searches, int32_t n_searches, const lba_s3p_point* points, int32_t n_points,
                           const uint8_t* taken, int32_t n_taken, lba_s3p_row* rows, int32_t n_rows,
                           int32_t* feat_point, int32_t n_feat_point, lba_s3p_pose* poses, int32_t n_poses,
                           const lba_s3p_params* prm);
/* Measurement only: on != 0 makes lba_match_sim3_project bracket its launches with events on the tracker's stream;
 * last_ms (may be NULL) receives {k_s3p_pose, k_s3p_project, k_s3p_compact + k_s3p_base, the readback and the host's
 * sizing, k_s3p_gather, k_s3p_resolve} of the last such call in milliseconds, or -1. */
int lba_match_sim3_project_profile(lba_tracker* t, int32_t on, double* last_ms /* [6] */);

/* ---- local mapping and loop closing: the SEARCH of ORBmatcher::Fuse, both overloads (src/ORBmatcher.cc:1133-1316 and
 * :1318-1437; LocalMapping::SearchInNeighbors, LoopClosing::SearchAndFuse), for a batch of searches.  Which feature a
 * (point, camera) picks, and at what distance, depends on the point's position, normal, distance range and descriptor
 * and on the keyframe's features, grid and camera poses, and on nothing else: neither overload keeps a vbMatched or
 * taken flag.  The map enters only in the skip in front (isBad, IsInKFCamera, spAlreadyFound) and in the decision
 * behind (GetMapPoint(bestIdx), Observations(), Replace / AddObservation / vpReplacePoint); both stay with the caller
 * (amc_lba.fuse.fuse_walk is that tail).  So this call writes one row per job and edits nothing.
 *
 * A *target* is a keyframe: its cameras (one lba_fuse_cam and one lba_match_cam each, at cam0 + c), its features
 * (numbered from 0 within the target, as cell_feat and `feat` number them), its own 64 x 48 CSR grid per camera as a
 * search of lba_match_project has it (cell0: its n_cam * 64 * 48 + 1 entries of cell_start, the first 0; cf0: its
 * entries of cell_feat), its pyramid (sf0 / sigma0: n_levels entries of scale_factors / inv_level_sigma2 each).
 * A *search* is one target, one range of `points` (ranges may be shared), a mode and th.  A *job* is one (search,
 * point, camera), in the reference's loop order: row `row0 + p * n_cam + c`.
 *
 * Per job, every float expression in FLOAT, in this order, without contraction, divide and square root correctly
 * rounded:
 *   p3Dc = vTcw[c] * p3Dw as Sophus' SO3::operator* (so3.hpp:358-367) on the float quaternion as stored:
 *     uv = qv x p (Eigen's order: a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); uv += uv;
 *     ((p + w * uv) + qv x uv) per component, then + t.  (Not the matrix form of lba_match_sim3_project.)
 *   z < 0 -> BEHIND; u = fx * X / Z + cx, v likewise (Pinhole::project); IsInImage (u >= min_x && u < max_x && ..)
 *   else OUT_OF_IMAGE; PO = p - ow[c], dist = sqrt((x^2 + y^2) + z^2); dist < min_dist || dist > max_dist -> DIST;
 *   (PO.x n.x + PO.y n.y) + PO.z n.z < 0.5f * dist -> ANGLE; PredictScale as lba_match_sim3_project's (clamped, its
 *   quirk (h)); radius = th * scale_factors[level]; GetFeaturesInArea's rectangle and window test; the candidates in
 *   ITS order (ix, then iy, then the cell's list); keypoint levels [level - 1, level].
 *   LBA_FUSE_KF (overload 1): every camera; ur = u - bf * (1.0f / Z); in the LAST camera a feature with u_right >= 0
 *     has e2 = (ex^2 + ey^2) + er^2 and is dropped when (double)(e2 * inv_level_sigma2[kpLevel]) > 7.8; every other
 *     feature e2 = ex^2 + ey^2 against 5.99 (the float product against the double literal, :1264 / :1275).  The best
 *     starts at 256 with strict <: a distance of 256 never wins and leaves feat -1.
 *   LBA_FUSE_SIM3 (overload 2): cameras 0 .. n_cam - 2; the last camera's rows are LBA_FUSE_NO_CAMERA.  No error gate.
 *     The best starts at INT_MAX: a distance of 256 can win (feat names it) and is then rejected.  ow[c] is the
 *     caller's vTcw[c].inverse().translation().
 *   accepted (LBA_FUSE_OK) when best_dist <= th_low, else LBA_FUSE_TOO_FAR; LBA_FUSE_NO_CAND when the window is empty
 *   or no candidate passed the level and error gates (best_dist 256, feat -1).
 * ONLY LBA_FUSE_OK and LBA_FUSE_TOO_FAR rows depend on the point's descriptor: every other status is decided before a
 * descriptor is read, and n_cand, level, x, y and radius never depend on it.  The caller's ordered walk rests on this:
 * a point whose descriptor an earlier Replace changed needs its OK / TOO_FAR rows redone and no others.
 * The call does NOT apply IsInKFCamera: every camera of every point whose `skip` is 0 is computed.  A point that
 * loses a Replace has its observations cleared, and the reference then searches cameras it would have skipped.
 * Quirks of the reference that are kept: (a) the last camera is skipped in overload 2; (b) Scw is unused there (:1328
 * is commented out); (c) the stereo test is u_right >= 0, zero counts; (d) z == 0 passes `z < 0` and ends
 * OUT_OF_IMAGE; (e) bRight is unused; (f) a point fused in camera c goes on to camera c + 1.
 * Device (lba_fuse.hip): ONE launch, k_fuse; a wave takes 64 consecutive jobs, lane = job for the projection and the
 * gates, then walks its live jobs one by one with all 64 lanes striding the window's spans.  No atomics, no LDS, no
 * wait on another workgroup; one upload, one download.  A row does not depend on the batch or on its position.
 * LBA_E_ARG: null tracker or arrays, a negative count, a target's n_cam < 1 or n_levels < 1, a target's camera,
 * feature, grid or pyramid range outside its array, a malformed grid (as lba_match_project), a search's target or
 * points outside their arrays, its rows outside `rows` or beginning before the end of the search before, a mode other
 * than the two, th negative or not finite, th_low negative.  LBA_E_LIMIT: n_cam > 64, more than LBA_MATCH_MAX_FEAT
 * features in one camera, an arena above 2 GB.  A refused call writes nothing and sets lba_tracker_last_error.
 * n_searches == 0, a search without points, a target without features and n_cam == 1 in LBA_FUSE_SIM3 (every row
 * LBA_FUSE_NO_CAMERA) are valid. */
#define LBA_FUSE_KF   0
#define LBA_FUSE_SIM3 1
#define LBA_FUSE_OK           0
#define LBA_FUSE_NO_CAND      1
#define LBA_FUSE_TOO_FAR      2
#define LBA_FUSE_SKIPPED      3
#define LBA_FUSE_BEHIND       4
#define LBA_FUSE_OUT_OF_IMAGE 5
#define LBA_FUSE_DIST         6
#define LBA_FUSE_ANGLE        7
#define LBA_FUSE_NO_CAMERA    8
#define LBA_FUSE_MAX_CAM      64
typedef struct lba_fuse_cam {      /* 72 bytes: one per (target, camera) */
    float   q_cw[4], t_cw[3];      /* mTcw[c]: the float unit quaternion as stored (x, y, z, w) and the translation */
    float   fx, fy, cx, cy;
    float   min_x, max_x, min_y, max_y;   /* mvMinX[c] .. mvMaxY[c] */
    float   ow[3];                 /* KF: GetCameraCenter(c); SIM3: vTcw[c].inverse().translation() */
} lba_fuse_cam;
typedef struct lba_fuse_target {   /* 48 bytes */
    int32_t cam0, n_cam;           /* its rows of `fcams` and `gcams` */
    int32_t feat0, n_feat;         /* its rows of `feats` */
    int32_t cell0, cf0;            /* its entries of `cell_start` and `cell_feat` */
    float   bf;                    /* mbf */
    float   log_scale_factor;      /* mfLogScaleFactor */
    int32_t n_levels;              /* mnScaleLevels */
    int32_t sf0, sigma0;           /* its n_levels entries of `scale_factors` and of `inv_level_sigma2` */
    int32_t pad;
} lba_fuse_target;
typedef struct lba_fuse_search {   /* 32 bytes */
    int32_t target;
    int32_t point0, n_points;      /* its range of `points` */
    int32_t row0;                  /* its n_points * n_cam rows of `rows` */
    int32_t mode;                  /* LBA_FUSE_KF / LBA_FUSE_SIM3 */
    float   th;
    int32_t n_ok;                  /* out: its LBA_FUSE_OK rows */
    int32_t pad;
} lba_fuse_search;
typedef struct lba_fuse_row {      /* out, 32 bytes: one job */
    int32_t status;                /* LBA_FUSE_* */
    int32_t feat;                  /* bestIdx, the target's keypoint index, or -1 */
    int32_t best_dist;             /* 256: none */
    int32_t level;                 /* nPredictedLevel, -1 for a job that failed a gate */
    float   x, y, radius;          /* uv and the radius; 0 where they were not reached */
    int32_t n_cand;                /* candidates that passed the window, level and error gates */
} lba_fuse_row;
int lba_match_fuse(lba_tracker* t, const lba_fuse_target* targets, int32_t n_targets, const lba_fuse_cam* fcams,
                   const lba_match_cam* gcams, int32_t n_cams, const float* scale_factors, int32_t n_scale_factors,
                   const float* inv_level_sigma2, int32_t n_inv_level_sigma2, const int32_t* cell_start,
                   int32_t n_cell_start, const int32_t* cell_feat, int32_t n_cell_feat, const lba_match_feat* feats,
                   int32_t n_feats, lba_fuse_search* searches, int32_t n_searches, const lba_s3p_point* points,
                   int32_t n_points, lba_fuse_row* rows, int32_t n_rows, int32_t th_low);
/* Measurement only: on != 0 makes lba_match_fuse bracket its launch with events on the tracker's stream; last_ms (may
 * be NULL) receives {k_fuse} of the last such call in milliseconds, or -1. */
int lba_match_fuse_profile(lba_tracker* t, int32_t on, double* last_ms /* [1] */);

/* ---- local mapping: MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:611-700) and
 * MapPoint::ComputeDistinctiveDescriptors (:498-578) for a batch of map points: what LocalMapping::ProcessNewKeyFrame
 * (:249-250), SearchInNeighbors (:687-688) and the tails of LocalGPBA / BundleAdjustment (Optimizer.cc:1416, :359) run
 * point by point.  They fill the fields the projection matchers gate on: lba_s3p_point's normal, min_dist, max_dist,
 * max_distance and desc.  A point's refresh reads its own position, observation list and reference keyframe, the
 * keyframes' features and camera centres, and nothing else: no state passes from point to point, so a batch is the
 * sequence exactly.
 *
 * The keyframe side is lba_match_epipolar's arrays as they are (a caller builds them once for match_epipolar,
 * triangulate and this call): lba_tri_kf gives cam0; lba_tri_cam gives Ow, GetCameraCenter(c) widened to double, which
 * is narrowed back to float here (exact for the map's values, which are floats; any other double is rounded to
 * nearest); lba_epi_kf gives feat0 / n_feat; lba_epi_feat gives cam, scale (mvScaleFactors[octave]) and desc, in the
 * keyframe's global keypoint order: the index :674 uses and, through mmpGlobalToLocalID, :534.  Nothing else of the
 * four is read.  kf_bad[k] != 0: keyframe k isBad(); NULL: none is.
 * obs: one entry per (keyframe, camera) observation: `feat` is the keyframe-local keypoint index, the camera is that
 * feature's `cam`.  A point lists its observations IN THE REFERENCE'S ITERATION ORDER: mObservations' order, cameras
 * ascending within a keyframe.  The float sum of the normal depends on that order and the device keeps it.
 *
 * Per point, ops bit 0 (normal and depth) and bit 1 (descriptor) select either function or both; neither reads what
 * the other writes.
 *   early     bad -> LBA_MP_BAD; n_obs == 0 -> LBA_MP_EMPTY; neither writes normal, min_distance, max_distance or desc.
 *   desc      the candidates are the observations whose keyframe is NOT bad, in list order (:521); N their count.
 *             N == 0: desc untouched, best_obs = best_median = -1.  Else the N x N matrix of 256-bit Hamming
 *             distances; per row the element at sorted position int(0.5 * (N - 1)): the LOWER median, the row's own 0
 *             included; the FIRST row with the strictly smallest median wins (:559-572).  desc = its descriptor,
 *             best_obs = its position in the point's list, best_median = its median.  All integers: exact.
 *   normal    over ALL observations in list order, bad keyframes included (:632-659), in FLOAT without contraction,
 *             divide and square root correctly rounded: d = pos - Ow; r = sqrtf((dx dx + dy dy) + dz dz);
 *             normal = normal + d / r (a true division per component); n++; at the end normal / (float)n.
 *   depth     maxDist = FLT_MIN, minDist = FLT_MAX; over the observations with kf == ref_kf in list order:
 *             maxDist = max(maxDist, r * scale), minDist = min(minDist, r * scale / scale_top) left to right, with
 *             std::max / std::min's comparisons (a NaN never replaces).  max_distance = maxDist, min_distance = minDist
 *             (the raw mfMaxDistance / mfMinDistance: the 1.2 / 0.8 of Get*DistanceInvariance are the caller's,
 *             amc_lba.mappoint.points_to_s3p).
 * Quirks of the reference that are kept: (a) the normal counts observations in bad keyframes, the descriptor skips
 * them; (b) the lower median, ties to the first row; (c) a position on a camera centre gives 0 / 0: a NaN normal;
 * (d) ref_kf == -1 (mpRefKF not among the observations) indexes an empty vector there, undefined behaviour; HERE it is
 * defined as the host adapter defines it: no camera, FLT_MIN / FLT_MAX stored, the normal still computed.
 * Device (lba_mappoint.hip): one upload, up to three launches, one download.  k_mp_geom: one lane per point walks
 * its list in order.  The host sorts the descriptor points by N: k_mp_desc_wave (N <= 64) one wave per point, lane i
 * holds candidate i, candidate j is broadcast; k_mp_desc_block (65 .. 1024) one 256-thread workgroup per point, the
 * descriptors in LDS.  Both find a row's median by bisection on the value (9 steps over 0..256).  No atomics, no wait
 * on another workgroup.  A point's result does not depend on the batch or on its position, and is bitwise
 * reproducible.
 * LBA_E_ARG: null tracker, arrays or params, a negative count, n_cam < 1, a keyframe's cameras or features outside
 * their arrays, a feature's cam outside [0, n_cam), an observation's kf outside [0, n_kf) or feat outside its
 * keyframe, a point's range outside `obs`, ref_kf outside [-1, n_kf), ops outside 1..3, a scale_top that is NaN.
 * LBA_E_LIMIT: n_cam > 64, more than LBA_MATCH_MAX_FEAT features in one camera of a keyframe, a point with more than
 * LBA_MP_MAX_OBS observations (the reference's float Distances[N][N] overruns an 8 MB stack near N = 1448), an arena
 * above 2 GB.  A refused call writes nothing and sets lba_tracker_last_error.  n_points == 0 is valid; point ranges
 * may overlap or be shared; `obs` is not written. */
#define LBA_MP_OK      0
#define LBA_MP_BAD     1
#define LBA_MP_EMPTY   2
#define LBA_MP_NORMAL  1           /* ops bit 0: UpdateNormalAndDepth */
#define LBA_MP_DESC    2           /* ops bit 1: ComputeDistinctiveDescriptors */
#define LBA_MP_MAX_OBS 1024
typedef struct lba_mp_obs { int32_t kf, feat; } lba_mp_obs;
typedef struct lba_mp_point {      /* 112 bytes */
    float    pos[3];               /* mWorldPos */
    float    normal[3];            /* in / out: mNormalVector */
    float    min_distance, max_distance;   /* in / out: mfMinDistance, mfMaxDistance (raw) */
    uint32_t desc[8];              /* in / out: mDescriptor */
    int32_t  ref_kf;               /* mpRefKF's index in kfs, or -1: quirk (d) */
    int32_t  obs0, n_obs;          /* its range of `obs` */
    int32_t  bad;                  /* isBad() */
    int32_t  ops;                  /* LBA_MP_NORMAL | LBA_MP_DESC */
    int32_t  n;                    /* out: the observation count of :656; 0 where the normal was not computed */
    int32_t  best_obs;             /* out: position in the point's list of the chosen descriptor, or -1 */
    int32_t  best_median;          /* out: its median, or -1 */
    int32_t  status;               /* out: LBA_MP_* */
    int32_t  pad[3];
} lba_mp_point;
typedef struct lba_mp_params { float scale_top; } lba_mp_params;   /* mvScaleFactors[mnScaleLevels - 1] */
int lba_mappoint_refresh(lba_tracker* t, lba_mp_point* points, int32_t n_points, const lba_mp_obs* obs, int32_t n_obs,
                         const lba_tri_kf* kfs, const lba_epi_kf* ekfs, int32_t n_kf, const lba_tri_cam* cams,
                         int32_t n_cam_rows, int32_t n_cam, const lba_epi_feat* feats, int32_t n_feats,
                         const int32_t* kf_bad /* may be NULL */, const lba_mp_params* prm);
/* Measurement only: on != 0 makes lba_mappoint_refresh bracket its launches with events on the tracker's stream;
 * last_ms (may be NULL) receives {k_mp_geom, k_mp_desc_wave, k_mp_desc_block} of the last such call in milliseconds
 * (about 0 for a kernel that was not launched), or -1. */
int lba_mappoint_refresh_profile(lba_tracker* t, int32_t on, double* last_ms /* [3] */);

/* ---- loop closing: the optimisation of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:1434-1717, called from
 * LoopClosing::CorrectLoop), a Sim3 pose graph.  One g2o::VertexSim3Expmap per vertex (types_seven_dof_expmap.h:48-94:
 * estimate Siw, S <- Sim3(update) S, tangent [omega; upsilon; sigma], update[6] = 0 under fix_scale) and one
 * g2o::EdgeSim3 per edge (:99-126): e = log(C S[v0] S[v1]^-1), C the measurement Sji, information I, no robust kernel;
 * Sim3::log with its four branches at eps = 1e-5 (sim3.h:148-230).  g2o's Levenberg (tau, max_trials, early_stop of the
 * tracker's lba_config) over a sparse Cholesky factorisation of the full system: no vertex is marginalised.  The
 * reference differentiates EdgeSim3 numerically (central differences of 1e-9 through oplus); the device computes the
 * analytic Jacobians J0 = Jl^-1(e) Ad(C), J1 = -Jl^-1(e) Ad(E).  The graph construction
 * (:1504-1660) and the write-back (:1669-1713) are the caller's: amc_lba.posegraph.essential_graph / write_back.
 *
 * Activity follows g2o: an edge whose two vertices are fixed is inactive; a vertex that no active edge touches is
 * inactive: it has no rows in H, b or dx and is never written.  na counts the active free vertices, in array order
 * (pass the vertices sorted by keyframe id for g2o's order).  Several fixed vertices, parallel edges on one pair and
 * both orientations are allowed; a block of H sums its edges' terms in edge order.  Under fix_scale the sigma row of
 * every block of H is exactly 0 + lambda and its step is 0.  Results are bitwise reproducible, and do not depend on
 * what the tracker ran before.
 *
 * LBA_E_ARG: null tracker or arrays, n_v < 1, n_e < 0, iterations < 0, an edge's vertex index outside [0, n_v),
 * v0 == v1, a vertex's or an edge's s not finite or <= 0, a lambda that is not finite.  LBA_E_EMPTY: no active edge.
 * LBA_E_LIMIT: more than 2^20 vertices or 2^22 edges, a graph whose lists and tiles of L exceed 6 GB of device memory,
 * or (lba_posegraph_linearize only) more than 2048 active free vertices, whose dense H would exceed 1.6 GB.  A refused
 * call writes nothing.
 *
 * lba_posegraph_optimize: lambda_init > 0 is the user lambda (the reference: 1e-16), <= 0 means tau max|H_ii|.  A
 * failed factorisation (a non-positive pivot) is a trial with chi2 = DBL_MAX: the state is untouched and lambda
 * grows.  Writes the active free vertices in place, `out` if not NULL, and returns the LM iterations run (>= 0).  The
 * accept / reject decision is taken on the host: one readback of three doubles per trial.
 * lba_posegraph_linearize: the active edges' errors (zero for an inactive edge), the dense H (no lambda) and b over the
 * active free vertices; each of the three may be NULL.  Returns na.
 * lba_posegraph_step: one damped step at `lambda`: dx [7 na], the trial vertices (the others copied from `v`) and
 * the trial's chi2; each may be NULL.  Returns na, or LBA_E_SOLVE when a pivot is not positive (nothing written).
 * lba_posegraph_plan_info: host only, no device.  info = {na, panels, tiles of L, fill-in tiles, launch levels,
 * dependent chain (panels), loop-closure tail (panels), dissection depth}.  Returns na. */
typedef struct lba_pg_vertex {
    double  q[4], t[3], s;  /* in / out: Siw, (x, y, z, w) */
    int32_t fixed, pad;
} lba_pg_vertex;
typedef struct lba_pg_edge {
    int32_t v0, v1;         /* e = log(C S[v0] S[v1]^-1) */
    double  q[4], t[3], s;  /* C: the measurement Sji */
} lba_pg_edge;
typedef struct lba_pg_stats {
    int32_t iterations, trials, solve_failures, result;   /* result: 0, or 1 when the last iteration ran out of trials */
    double  chi2_initial, chi2_final, lambda_final;
    int32_t panels, tiles, fill_tiles, levels, chain, launches_per_solve;
} lba_pg_stats;
int lba_posegraph_optimize(lba_tracker* t, lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                           int32_t fix_scale, int32_t iterations, double lambda_init, lba_pg_stats* out);
int lba_posegraph_linearize(lba_tracker* t, const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                            int32_t fix_scale, double* errors /* [7 n_e] */, double* H /* [7 na x 7 na] */,
                            double* b /* [7 na] */);
int lba_posegraph_step(lba_tracker* t, const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e,
                       int32_t fix_scale, double lambda, double* dx /* [7 na] */, lba_pg_vertex* trial /* [n_v] */,
                       double* chi2_trial);
int lba_posegraph_plan_info(const lba_pg_vertex* v, int32_t n_v, const lba_pg_edge* e, int32_t n_e, int32_t info[8]);
/* Measurement only: the host planning, upload and device (first launch to last readback) milliseconds of the
 * tracker's last lba_posegraph_optimize. */
int lba_posegraph_profile(lba_tracker* t, double ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* AMC_LBA_H */
