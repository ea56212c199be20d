/* bodyfit.h — C ABI of the MI355X-native SMPL residual/Jacobian evaluator (libbodyfit.so).
 *
 * Drop-in boundary for the hot path of jonH34400/3DBodyAnimation: everything the reference
 * executes inside ceres::Solve's iteration loop (CostFunction::Evaluate of its residual blocks)
 * plus the SMPL forward (ark::Avatar::update) those blocks are defined on.  Plain pointers and
 * sizes only; no C++/torch types.  Every entry point returns 0 on success and a non-zero
 * bodyfit_status otherwise (Ceres convention: Evaluate()==false marks an infeasible step, so a
 * HIP failure maps to "false", never to an exception).  bodyfit_last_error() gives the text.
 *
 * Reference interfaces replaced (paths relative to the reference repository):
 *   bodyfit_model_*            ark::AvatarModel (external/avatar, absent) as used at
 *                              include/Sim3BA.h:360-372, include/MultiFrameBA.h:46-60;
 *                              tensors = SMPL npz keys (scripts/npz_fixer.py:4-17)
 *   bodyfit_gmm_*              ark::GaussianMixture (include/Sim3BA.h:249,257,266,280,288);
 *                              data format scripts/convert_gmm_to_avatar.py:14-29
 *   bodyfit_problem_create     the residual blocks added by include/Sim3BA.h:410-470,572-638 and
 *                              include/MultiFrameBA.h:71-142 (PixelKP list include/Sim3BA.h:9)
 *   bodyfit_evaluate_batch     one sweep of CostFunction::Evaluate over all those blocks:
 *                              ReprojCost / ReprojCostShape (include/Sim3BA.h:34-88,126-227) with an
 *                              analytic Jacobian in place of DynamicAutoDiffCostFunction (:420,581),
 *                              PosePriorAAAnalytic (:263-315), ShapePriorL2Analytic (:331-343),
 *                              Vec3DiffCost (include/MultiFrameBA.h:20-28)
 *   bodyfit_evaluate_block     ceres::CostFunction::Evaluate(parameters, residuals, jacobians)
 *                              for ONE block, same null conventions (include/Sim3BA.h:263-264)
 *   bodyfit_forward            ark::Avatar::update() (include/Sim3BA.h:371,538;
 *                              include/MultiFrameBA.h:53,173; src/main_single_frame.cpp:213,254)
 *   bodyfit_mean_pixel_error   mean_pixel_error (include/Utils.h:102-115)
 *   bodyfit_writeback_batch    the post-solve write-back loops (include/MultiFrameBA.h:154-174,
 *                              include/Sim3BA.h:481-505) + mean_pixel_error, for all frames at once
 *   bodyfit_reduce_shared_device  the shared shape block of OptimizeMultiFrame (include/MultiFrameBA.h:67-68)
 *                              reduced per GPU for frame-sharded solves
 *   bodyfit_frame_normals      per-frame normal equations of the reprojection blocks (what DENSE_QR
 *                              factors, include/MultiFrameBA.h:145-151), for structured window solvers
 *   bodyfit_solve              ceres::Solve as configured by OptimizePoseReprojection /
 *                              OptimizePoseShapeReprojection (include/Sim3BA.h:472-479,641-647) and
 *                              OptimizeMultiFrame (include/MultiFrameBA.h:144-151); the three functions
 *                              themselves are mirrored in include/bodyfit.hpp
 */
/* Environment variables the library reads.  None is needed in production; none changes a result (the A/B forms are tested
 * bit-identical to the default), they select between equivalent code paths for measurements and tests:
 *   BODYFIT_ONE_LAUNCH=0     problems created afterwards sweep as two launches (k_frame_resjac, k_mesh_blend_lbs) instead of one
 *   BODYFIT_LM_PLAIN=1       the batched LM in its four-launch form (step, residual sweep, accept, Jacobian sweep)
 *   BODYFIT_PACKED_J=0       bodyfit_evaluate_batch's cache keeps the dense Jacobian panel instead of the packed blocks
 *   BODYFIT_PACK_DIRECT=0    the packed Jacobian goes down by hipMemcpyAsync instead of by the packing kernel's own stores
 *   BODYFIT_FORCE_SHARDED=1  a one-rank communicator still takes the sharded code path (how RCCL is exercised on a one-GPU box)
 *   BODYFIT_WINDOW_MIN=n     shared-beta windows shorter than n frames iterate on the host (default 12)
 *   BODYFIT_HOST_NORMALS=1   the host loop builds its normal equations on the host; BODYFIT_TIMING=1 prints its phase times
 * The tuning words of the one-launch sweep (mesh priority, operand pacing, Jacobian store scope) are compile-time constants since
 * round 5 (csrc/bodyfit_device.h kTune*); round 4 read them from BODYFIT_MESH_PRIO / BODYFIT_TRICKLE_* / BODYFIT_J_SCOPE. */
#ifndef BODYFIT_H_
#define BODYFIT_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum bodyfit_status {
  BODYFIT_OK = 0,
  BODYFIT_ERR_INVALID = 1,   /* bad argument / shape                                  */
  BODYFIT_ERR_HIP = 2,       /* a HIP runtime call failed (no device, OOM, fault ...) */
  BODYFIT_ERR_NUMERIC = 3    /* non-SPD covariance etc.                               */
} bodyfit_status;

typedef struct bodyfit_model bodyfit_model;     /* device-resident SMPL model            */
typedef struct bodyfit_gmm bodyfit_gmm;         /* device-resident max-mixture pose prior */
typedef struct bodyfit_problem bodyfit_problem; /* residual blocks of one solve           */

/* SMPL tensors, host pointers, row-major f64 (the reference keeps Eigen doubles).          *
 * Accepted model shapes: any n_verts; 1 <= n_joints <= 24; 0 <= n_shape <= 10; n_pose_feat 0 or 9 (n_joints - 1);    *
 * a topologically ordered tree at most 13 levels deep below the root (deeper: BODYFIT_ERR_INVALID).  A frame's          *
 * parameter row is 7 + 3 (n_joints - 1) wide (76 for 24 joints).  Below 24 joints only the frame role is built:          *
 * keypoint residuals, Jacobian, joints, temporal rows, shape prior and the joints-only VJP; the pose prior               *
 * (beta_pose > 0), the mesh path (want_mesh, the cloud VJP) and the solvers need 24 joints.                          */
typedef struct bodyfit_model_desc {
  int n_verts;               /* 6890 */
  int n_joints;              /* 24   */
  int n_shape;               /* 10   */
  int n_pose_feat;           /* 207 = 9 (n_joints-1); 0 disables pose-corrective blendshapes */
  const double* v_template;  /* [n_verts][3]              */
  const double* shapedirs;   /* [n_verts][3][n_shape]     */
  const double* posedirs;    /* [n_verts][3][n_pose_feat] or NULL */
  const double* j_regressor; /* [n_joints][n_verts]       */
  const double* weights;     /* [n_verts][n_joints]       */
  const int* parent;         /* [n_joints], root = -1 (scripts/npz_fixer.py); parent[j] < j; depth <= 13 */
  int n_landmarks;           /* vertex-landmark keypoints (0 = none) */
  const int* landmark_vid;   /* [n_landmarks] vertex ids  */
  /* Sparse keypoint regressors over the POSED vertices (0 = none): keypoint id n_joints + n_landmarks + r is
   *   sum_i kpreg_weight[i] * posed_vertex(kpreg_vid[i]),  i in [kpreg_offset[r], kpreg_offset[r + 1])
   * (OpenPose-style extra keypoints: a weighted mean of a few surface vertices; the avatar library's keypoints of this
   * kind are what the reference's PixelKP::jid would address past the 24 SMPL joints, include/Sim3BA.h:28-33).
   * Evaluated exactly, with its Jacobian, in the frame kernel: per skinning joint j the row collapses to ONE pseudo-vertex
   * (sum_i w_i W_ij [v_i ; 1] is linear in the vertex rows), so a row costs as many landmark slots as its vertices have
   * distinct joints.  Landmarks + slots of all rows <= 32.                                                               */
  int n_kp_regressors;
  const int* kpreg_offset;    /* [n_kp_regressors + 1] */
  const int* kpreg_vid;       /* [nnz] vertex ids      */
  const double* kpreg_weight; /* [nnz]                 */
} bodyfit_model_desc;

int bodyfit_model_create(const bodyfit_model_desc* desc, int device, bodyfit_model** out);
void bodyfit_model_destroy(bodyfit_model* m);
/* initialJointPos [nJ][3], jointShapeReg [3 nJ][nS], rest offsets [nJ][3] (include/Sim3BA.h:372-392),
 * regressed on the device at create time.  Any pointer may be NULL.                         */
int bodyfit_model_get_derived(const bodyfit_model* m, double* joints0, double* joint_shape_reg,
                              double* offset);

/* pose_prior.txt contents: K weights, K x D means, K x D x D covariances (row-major).
 * resid_scale: factor on L_k^T (x - mu_k) inside residual(); sqrt(0.5) = recalled upstream.  */
int bodyfit_gmm_create(int n_comp, int dim, const double* weights, const double* means,
                       const double* covs, double resid_scale, int device, bodyfit_gmm** out);
void bodyfit_gmm_destroy(bodyfit_gmm* g);
/* prec_cho [K][D][D] (lower L, precision = L L^T) and -log of the normalised weights [K]. */
int bodyfit_gmm_get(const bodyfit_gmm* g, double* prec_cho, double* neg_log_w);

/* Frame parameter packing (order is load-bearing, include/Sim3BA.h:36-40,421-430):
 *   x[76] = [scale, rootAA(3), rootT(3), jointAA[1](3) ... jointAA[23](3)]                  */
#define BODYFIT_FRAME_PARAMS 76

typedef struct bodyfit_problem_desc {
  int n_frames;
  const int* kp_offset;   /* [n_frames+1] CSR over keypoints (frames may be empty)            */
  const int* kp_id;       /* [K] id < n_joints: SMPL joint (PixelKP::jid);
                                 n_joints <= id < n_joints + n_landmarks: vertex landmark id - n_joints;
                                 above: keypoint regressor row id - n_joints - n_landmarks    */
  const double* kp_uv;    /* [K][2] observed pixels (PixelKP::u,v)                            */
  double fx, fy, cx, cy;
  const double* R0;       /* [n_frames][9] row-major fixed root orientation (avatar.r[0])     */
  int n_cols;             /* 76: blocks of ReprojCost; 76+n_shape: + the shape block          */
  int use_shape;          /* jointShapeReg handed to the functor (betaShape > 0); else the
                             shape block, if present, gets zero columns (MultiFrameBA.h:88)   */
  int beta_per_frame;     /* 0: one shared beta[n_shape]; 1: beta[n_frames][n_shape]          */
  int pose_blend;         /* apply posedirs in vertex landmarks and the mesh                  */
  double beta_pose;       /* PosePriorAAAnalytic weight; 0 = no prior block (> 0 needs 24 joints) */
  const bodyfit_gmm* gmm; /* NULL = L2 fallback (include/Sim3BA.h:283)                        */
  double beta_shape;      /* ShapePriorL2Analytic weight; 0 = none                            */
  double lambda_temporal; /* Vec3DiffCost weight between frames f, f+1; 0 = none              */
  int temporal_halo;      /* 1: frame_params holds n_frames+1 rows; the last row is the next
                             shard's first frame and only feeds the last temporal block       */
  double huber_delta;     /* HuberLoss on reprojection blocks (3.0 in the reference)          */
  int want_mesh;          /* also produce the 6890-vertex cloud per frame on each evaluation  */
} bodyfit_problem_desc;

/* Synchronous: allocates and uploads the problem's device state and clears what needs clearing on the NULL stream, and waits
 * for those clears before it returns, so that the problem's first caller may be on any stream (a non-blocking stream is not
 * ordered against the NULL stream).  A window solve that has to grow its pool clears it and waits in the same way, once. */
int bodyfit_problem_create(const bodyfit_model* m, const bodyfit_problem_desc* desc, bodyfit_problem** out);
void bodyfit_problem_destroy(bodyfit_problem* p);

/* Row layout of the batched residual vector (bodyfit_problem_layout):
 *   [reproj: 2 per keypoint, frame-major][pose prior: n_prior_rows per frame]
 *   [shape prior: n_shape per beta][temporal: 75 per adjacent pair: rootT, rootAA, joints 1..23]
 * The reprojection Jacobian is a dense row-major [2K][n_cols] panel (columns = the frame's 76
 * parameters, then beta).  Prior/temporal Jacobians are constant (beta I, beta_p L_k^T, +-lambda I)
 * and are reproduced by bodyfit_evaluate_block / the host solver from gmm_comp.               */
typedef struct bodyfit_layout {
  int n_keypoints;      /* K                                  */
  int n_cols;
  int reproj_rows;      /* 2 K                                */
  int prior_rows_per_frame; /* 0, 69 (L2) or 70 (GMM)         */
  int shape_rows;       /* 0, nS or F nS                      */
  int temporal_rows;    /* 0 or 75 (F-1 [+1 with halo])       */
  int total_rows;
} bodyfit_layout;
int bodyfit_problem_layout(const bodyfit_problem* p, bodyfit_layout* out);

/* Host-pointer form: H2D of the parameters, one device sweep, D2H of the results.
 *   frame_params [F(+1)][76], beta [nS] or [F][nS] (NULL if n_cols == 76)
 *   residuals [total_rows]; jacobian [2K][n_cols] or NULL (want_jacobian = 0);
 *   gmm_comp [F] or NULL: selected mixture component per frame.                               */
int bodyfit_evaluate_batch(bodyfit_problem* p, const double* frame_params, const double* beta,
                           double* residuals, double* jacobian, int* gmm_comp, int want_jacobian);

/* Device-pointer form (inputs already resident in HBM, asynchronous on `stream`, a hipStream_t
 * passed as void*; NULL = the default stream).  Results stay in the problem's device buffers.
 * One problem, one sweep at a time: successive calls must be ordered (same stream, or events); the synchronous entry points
 * (bodyfit_evaluate_batch, bodyfit_forward, bodyfit_writeback_batch, bodyfit_frame_normals) order themselves behind whatever
 * was enqueued through this call (they run on a private stream / the NULL stream).
 * Errors of an asynchronous sweep.  With want_mesh the sweep is ONE launch whose mesh workgroups wait, inside the launch, for
 * operands the frame workgroups publish (k_sweep.hip).  Every such wait is bounded; a mesh workgroup whose wait runs out leaves
 * its 32-vertex tile of the cloud unwritten and sets an error word.  Residuals, Jacobian, joints, GMM components and the
 * shared reduction (bodyfit_reduce_shared_device / bodyfit_arm_shared_reduction) never depend on a wait and are complete
 * regardless.  The synchronous entry points notice the word and re-issue their sweep as two launches themselves; a caller of
 * THIS function learns of it from bodyfit_sweep_status, which it should call before it consumes the cloud.             */
int bodyfit_evaluate_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                            int want_jacobian, void* stream);
/* Waits for `stream`, then reports whether every asynchronous sweep of the problem since the last check completed:
 * BODYFIT_OK, or BODYFIT_ERR_HIP ("... timed out"): the cloud of at least one of them is incomplete; the problem uses the
 * two-launch sweep from then on, so re-issuing the evaluation gives the complete result.                                */
int bodyfit_sweep_status(bodyfit_problem* p, void* stream);
/* One-launch sweeps of this problem found incomplete (an in-launch wait ran out) since it was created, whoever noticed: a
 * synchronous entry point that re-issued its sweep, or bodyfit_sweep_status.  0 in every healthy run; benchmarks report it. */
long bodyfit_sweep_timeouts(const bodyfit_problem* p);
/* Lifetime of `stream`: the synchronous entry points and the device solves order themselves behind the last asynchronous call
 * by recording an event ON THAT STREAM, so it must stay alive until the problem's next synchronous call (or
 * bodyfit_sweep_status on it) has returned. */

typedef struct bodyfit_device_views {
  double* residuals;    /* [total_rows]          */
  double* jacobian;     /* [2K][n_cols]          */
  int* gmm_comp;        /* [F]                   */
  float* cloud;         /* [F][cloud_frame_stride] f32, camera frame (want_mesh): frame f's
                           [n_verts][3] block starts at cloud + f * cloud_frame_stride          */
  double* joints;       /* [F][n_joints][3] camera-frame posed joints             */
  double* normal_eq;    /* [66] see bodyfit_reduce_shared_device                  */
  long long cloud_frame_stride; /* floats; 3 n_verts rounded up to whole 32-vertex tiles (a multiple of
                           128 bytes, so that every wave of the mesh kernel stores whole cache lines)     */
} bodyfit_device_views;
int bodyfit_problem_views(bodyfit_problem* p, bodyfit_device_views* out);

/* Shared-shape reduction for frame-sharded solves: after an evaluation, reduce over the local
 * frames  out[0] = cost = sum 1/2 rho(|r|^2) (+ 1/2 |r|^2 of the prior/temporal rows),
 *         out[1..10] = g_beta = sum J_beta^T (rho' r),  out[11..65] = upper(H_bb) = sum rho' J_beta^T J_beta.
 * d_out66 (device, 66 doubles) is what the caller all-reduces across ranks (RCCL).            */
int bodyfit_reduce_shared_device(bodyfit_problem* p, double* d_out66, void* stream);
/* Arm the reduction: every following Jacobian sweep of this problem (want_jacobian, want_mesh, shared beta, at most
 * 256 frames + prior tiles: a shard of a sharded window) deposits the 66 doubles in d_out66 at ITS OWN TAIL — the last
 * frame workgroup to finish sums the per-frame partials while the mesh workgroups are still running — and
 * bodyfit_reduce_shared_device(p, d_out66, stream) on the same stream then launches nothing.  Sweeps that cannot fold
 * (two-launch sweep, longer shards) leave the work to bodyfit_reduce_shared_device as before; the numbers are
 * bit-identical either way.  d_out66 = NULL disarms.                                                             */
int bodyfit_arm_shared_reduction(bodyfit_problem* p, double* d_out66);
/* (A timed-out in-launch wait — see bodyfit_evaluate_device — does not touch the 66 doubles: the frame and prior workgroups
 *  that produce them wait for nothing they need.)                                                                  */

/* Measurement aid: `iters` sweeps with HIP events around every kernel on `stream`;
 * avg_ms[5] = average launch duration (ms) of {frame_resjac, 0 (the prior workgroups ride on another launch),
 * mesh_blend_lbs, reduce_shared, sweep_roles}.  A sweep with the mesh on is ONE launch (sweep_roles: frame, mesh and prior
 * workgroups side by side); then entries 0 and 2 are 0.  Without the mesh, or with BODYFIT_ONE_LAUNCH=0, entry 4 is 0.
 * Entry 3 is ~0 when the reduction rode on the sweep's own tail (bodyfit_arm_shared_reduction). */
int bodyfit_profile_sweep(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                          int want_jacobian, int with_reduce, int iters, void* stream, double* avg_ms);

/* ceres::CostFunction::Evaluate for ONE residual block, Ceres pointer conventions
 * (jacobians may be NULL; jacobians[b] may be NULL; blocks row-major num_residuals x size).
 *   kind 0: reprojection block `index` (keypoint), parameters = 26 or 27 blocks
 *   kind 1: pose prior of frame `index`, parameters = 23 blocks of 3
 *   kind 2: shape prior (index = frame when beta_per_frame), parameters = 1 block of nS
 *   kind 3: temporal link `index` = 25*pair + slot, parameters = 2 blocks of 3                */
int bodyfit_evaluate_block(bodyfit_problem* p, int kind, int index, const double* const* parameters,
                           double* residuals, double** jacobians);

/* The same, for callers that follow ceres::EvaluationCallback (bodyfit_ceres::SweepCallback): the cached sweep is trusted to be
 * the point under evaluation, so reprojection / pose-prior blocks are served without comparing their parameters with the cache
 * and without a lock (Ceres evaluates blocks on several threads).  Fails if no sweep is cached.                           */
int bodyfit_evaluate_block_cached(bodyfit_problem* p, int kind, int index, const double* const* parameters,
                                  double* residuals, double** jacobians);

/* ark::Avatar::update(): camera-frame joints [F][nJ][3] (f64) and cloud [F][V][3] (f32) for the
 * problem's frames at the given parameters; either output may be NULL.
 * PRECISION.  Joints (f64): 1e-11 max(1, M_f / 4) m, M_f the frame's largest |coordinate| in metres.  Cloud (f32), per
 * frame, against the exact forward of the f64 inputs:   |cloud_fv - exact| <= B_f = 4 E_f,   with E_f the largest error over
 * the frame's vertices of the stated arithmetic itself on that frame: blend coefficients vec(R_j - I) in f32 (the one-launch
 * sweep: Rodrigues in f32 from the parameters rounded to f32, first-order branch at theta^2 <= 1e-20; the two-launch sweep:
 * the f64 rotation rounded to f32), beta and the model's directions in f32; both operands split in bf16 hi + lo by
 * round-to-nearest-even, hi.hi + hi.lo + lo.hi accumulated in f32; the skinning transforms s Rr0 [A_j | P_j - A_j Jc_j] +
 * [0 | t] computed in f64 and rounded to f32; the blend of a vertex's <= 4 transforms and the 3 x 4 product in f32.
 * tests/domain_cases.py (model_cloud) is that arithmetic in numpy and tabulates E_f; the factor 4 covers the order of the f32
 * sums and fused against unfused products.  E_f is about 1.5 f32 ulps of the frame's largest coordinate (the translation is
 * inside the transform: 6e-7 m at 3 m, 1.6e-5 m at 100 m) plus about 2^-19 |s| (sum_k |feat_k| |posedirs_vk| + sum_k |beta_k|
 * |shapedirs_vk|) (3.6e-6 m at |beta| = 5; 8.5e-5 m at theta = pi, |beta| = 5, s = 20, t_z = 60).  For |t| <= 4 m, s <= 1.4,
 * |beta| ~ 1 this is the 5e-6 m the contract used to state in metres alone.  The clouds of the two sweeps lie within 2 B_f
 * of each other (2e-6 m on such inputs).                                                                              */
int bodyfit_forward(bodyfit_problem* p, const double* frame_params, const double* beta,
                    double* joints, float* cloud);

/* Device-pointer form of bodyfit_forward into caller memory, asynchronous on `stream` (no host synchronisation):
 *   d_frame_params [F(+1)][76], d_beta [nS] or [F][nS] (NULL: beta = 0), d_joints [F][nJ][3] f64 or NULL,
 *   d_cloud [F][cloud_row_floats] f32 (cloud_row_floats >= 3 V; needs want_mesh) or NULL.
 * Always the two-launch sweep (k_frame_resjac, then k_mesh_blend_lbs: no in-launch waits, so no bodyfit_sweep_status
 * round trip), which is the sweep bodyfit_forward_vjp* differentiates: its cloud is bodyfit_forward's with the one-launch
 * sweep switched off (BODYFIT_ONE_LAUNCH=0) bit for bit, and within 2e-6 of the one-launch sweep's.  Ordered like
 * bodyfit_evaluate_device (it uses the problem's sweep buffers).                                                      */
int bodyfit_forward_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, double* d_joints,
                           float* d_cloud, long long cloud_row_floats, void* stream);

/* Reverse-mode gradient (vector-Jacobian product) of that forward: given the upstream gradients
 *   d_grad_cloud  [F][grad_cloud_row_floats] f32 = dL/dcloud (needs want_mesh) or NULL,
 *   d_grad_joints [F][nJ][3] f64 = dL/djoints or NULL,
 * writes d_grad_frame_params [F(+1)][76] f64 = dL/dframe_params (the halo row of a temporal_halo problem: 0) and
 * d_grad_beta = dL/dbeta, [nS] summed over the frames when beta is shared, [F][nS] when beta_per_frame (required when
 * n_cols = 76 + nS; with n_cols = 76 it may be NULL, otherwise it receives zeros; zeros too without use_shape).
 * Under the problem's use_shape / pose_blend / beta_per_frame and its fixed R0.  Asynchronous on `stream`, ordered like
 * bodyfit_evaluate_device; uses buffers of its own (allocated on the problem's first VJP, and the model's transposed
 * operand block on the model's first VJP: that first call synchronises once), so it leaves the sweep buffers alone.
 * Deterministic: no atomics, fixed summation orders; a frame's rows depend on that frame only (bit-identical whatever F).
 * Without d_grad_cloud only the f64 chain kernel runs (problems without want_mesh included).
 * PRECISION, per entry (frame f, column c), with S_fc = sum_i |G_fi| |dcloud_fi / dx_c| + sum |H| |djoints / dx_c|: within
 * 2^-14 S_fc of the exact gradient with d_grad_cloud (each operand of the bf16 hi + lo split carries 16 significant bits, a
 * product term is off by at most 2^-15 relative; a factor 2 for the f32 accumulation and the f32 skinning adjoint), within
 * 1e-9 S_fc without it (f64 throughout) -- and also within 1e-4 (1e-7) of the frame's largest entry.  One exception, by
 * design: a rotation with 0 < theta^2 <= DBL_EPSILON takes R = I + [a]x and dR_c = [e_c]x (the reference's Ceres branch;
 * sweep, VJP and JVP alike), which is off the exponential's derivative by up to 2 theta <= 3e-8 per entry: the three columns
 * of such a rotation carry up to 2 theta D_f sum |H_f| more, D_f the diameter of the posed skeleton in metres.
 * BODYFIT_ERR_INVALID: NULL problem / parameters / d_grad_frame_params, grad_cloud without want_mesh or with a row
 * shorter than 3 V, d_grad_beta missing with n_cols = 76 + nS.                                                          */
int bodyfit_forward_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                               const float* d_grad_cloud, long long grad_cloud_row_floats, const double* d_grad_joints,
                               double* d_grad_frame_params, double* d_grad_beta, void* stream);
/* Host-pointer form of bodyfit_forward_vjp_device (same shapes, grad_cloud rows of 3 V floats), synchronous. */
int bodyfit_forward_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const float* grad_cloud,
                        const double* grad_joints, double* grad_frame_params, double* grad_beta);

/* Forward-mode tangents (Jacobian-vector products) of that forward, n_tangents = K per frame at once: given
 *   d_tan_params [F][K][76] f64 = the tangents of the frame parameters (order [s, rootAA, rootT, jointAA[1..]]; NULL: 0; a
 *                temporal_halo problem's extra parameter row is read past and has no tangent),
 *   d_tan_beta   [K][nS] f64 when beta is shared, [F][K][nS] when beta_per_frame (NULL: 0; ignored with n_cols = 76),
 * writes the directional derivatives of exactly what bodyfit_forward_device computes,
 *   d_tan_joints [F][K][nJ][3] f64 or NULL,   d_tan_cloud [F][K][row_floats] f32 (row_floats >= 3 V; needs want_mesh) or NULL,
 * under the problem's use_shape / pose_blend / beta_per_frame and its fixed R0 (without pose_blend the pose features carry no
 * tangent, without use_shape beta carries none).  With the 76 + nS unit tangents the outputs are the dense Jacobian.
 * Tolerances (against central differences of the f64 forward): joints <= 1e-7, cloud <= 1e-4 of the largest entry of that
 * (frame, tangent)'s tangent (unit tangents included: every column of the Jacobian to its own scale; the joints' plus
 * 2 theta D_f on the columns of a rotation in the first-order branch, see bodyfit_forward_vjp_device); the chain is f64, the blend tangent runs on the matrix pipe like the forward's blend (bf16 hi/lo
 * split, f32 accumulation) and the skinning tangent is f32.
 * Deterministic: no atomics, fixed summation orders; the outputs of (frame, tangent) depend on that frame's parameters and that
 * tangent only (bit-identical whatever F and K and wherever the tangent sits); a zero tangent gives exactly 0.
 * Memory: buffers of its own, allocated on the problem's first JVP with d_tan_cloud and freed with the problem (about 2.8 MB per
 * frame whatever K: one tile of 32 tangents per frame, the tiles run one after the other); the sweep buffers, the dense-Jacobian
 * flag and the VJP's buffers are left alone.  Without d_tan_cloud only the f64 chain kernel runs and nothing is allocated
 * (problems without want_mesh and models with n_joints != 24 included).
 * Asynchronous on `stream`, ordered like bodyfit_evaluate_device.
 * BODYFIT_ERR_INVALID: NULL problem / parameters, n_tangents < 1, both outputs NULL, d_tan_cloud without want_mesh or with
 * row_floats < 3 V.                                                                                                       */
int bodyfit_forward_jvp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, int n_tangents,
                               const double* d_tan_params, const double* d_tan_beta, double* d_tan_joints, float* d_tan_cloud,
                               long long row_floats, void* stream);
/* Host-pointer form of bodyfit_forward_jvp_device (same shapes, tan_cloud rows of 3 V floats), synchronous. */
int bodyfit_forward_jvp(bodyfit_problem* p, const double* frame_params, const double* beta, int n_tangents,
                        const double* tan_params, const double* tan_beta, double* tan_joints, float* tan_cloud);

/* ---- per-vertex offsets (SMPL+D) -------------------------------------------------------------------------------------------
 * A displacement d_v per vertex, added to the blended rest vertex before skinning (k_offsets.hip):
 *   cloud_v = sum_j W_vj T_j [b_v + d_v; 1] = cloud0_v + L_fv d_v,   L_fv = sum_j W_vj T_j[:, :3] = s Rr0 (blended rotations),
 * cloud0 = bodyfit_forward_device's cloud.  T_j, b_v and the JOINTS are those of the undisplaced shape (the usual SMPL+D
 * convention: the joints are regressed from template + shapedirs beta, so d_joints, the keypoint landmarks, the one-launch sweep
 * and the solvers do not see d).  L_fv does not depend on beta.
 *   d_offsets f32: [V][3] shared by the frames (offsets_frame_stride = 0), or frame f's [V][3] at d_offsets + f
 *   offsets_frame_stride (>= 3 V).  NULL: every function below IS the function it extends, launch for launch (the functions
 *   above call these with NULL).  Offsets need the mesh path: a want_mesh problem and a model with 24 joints; a call without its
 *   cloud argument (d_cloud / d_grad_cloud / d_tan_cloud) ignores valid offsets, since nothing else depends on them.
 * bodyfit_forward_offsets_device: the two-launch forward into the caller's rows, then k_offsets_apply on those rows: one
 *   thread per (frame, vertex) blends the vertex's four transforms (the f32 ones the forward left behind, the frame's 24 x 12
 *   floats staged once per workgroup) as the VJP's k_vjp_vertex_grad does and adds L_fv d_v in place.  A vertex with d_v == 0 is
 *   not touched, so zero offsets give bodyfit_forward_device's cloud bit for bit.  Frame-independent (frame f's rows are
 *   bit-identical whatever F).  Error against the exact delta = L_fv d_v, per component, both clouds from the device:
 *     |cloud_d - cloud0 - delta| <= 2^-24 (16 |s| |d_v|_1 + |cloud_d|):
 *   every entry of L is <= |s| in magnitude and carries the rounding of its f32 transform entries (1), of the weights (1), of
 *   the four blend products and sums (4, fewer where the compiler fuses) and of the three products and two sums with d (3 at
 *   most counted against |s| |d_v|_1): about 9 u |s| |d_v|_1, u = 2^-24; the final sum cloud0 + delta rounds once, u |cloud_d|.
 * bodyfit_forward_offsets_vjp_device: bodyfit_forward_vjp_device of the displaced forward.  k_offsets_displace adds d to the
 *   blended rest vertices between stage a and stage c, so dL/dT_j = sum_v W_vj G_v [b_v + d_v; 1]^T; stage b's input gb_v =
 *   L_fv^T G_v does not depend on d and is untouched.  d_grad_offsets (f32, the layout and stride of d_offsets; NULL: not wanted)
 *   receives dL/dd: per-frame offsets gb_fv itself, shared offsets sum_f gb_fv, the frames added in ascending order in f64 and
 *   rounded once (no atomics: bit-identical from run to run, and equal to that sum of the per-frame result bit for bit).
 *   Error against the exact sum_f L_fv^T G_fv per component: <= 2^-24 (16 sum_f |s_f| |G_fv|_1 + |dL/dd|), by the count above
 *   with G in the place of d, plus the one final rounding.  Rows of d_grad_offsets longer than 3 V: the rest is not written.
 *   d_grad_offsets without d_grad_cloud is BODYFIT_ERR_INVALID (chosen over writing zeros: a gradient on the joints alone does
 *   not reach the offsets, and a caller who asks for it has most likely dropped an argument).
 * bodyfit_forward_offsets_jvp_device: bodyfit_forward_jvp_device at the displaced point; the same displace kernel between the
 *   primal blend and the skinning tangent, clouddot_v = sum_j W_vj (Tdot_j [b_v + d_v; 1] + T_j[:, :3] bdot_v).  The offsets are
 *   constants: they carry no tangent.  Tolerances as bodyfit_forward_jvp_device.
 * Otherwise each takes the arguments, ordering rules and errors of the function it extends, and in addition
 * BODYFIT_ERR_INVALID: offsets without want_mesh, offsets with n_joints != 24, a stride in (0, 3 V), d_grad_offsets without
 * d_offsets or without d_grad_cloud.                                                                                       */
int bodyfit_forward_offsets_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, const float* d_offsets,
                                   long long offsets_frame_stride, double* d_joints, float* d_cloud, long long cloud_row_floats,
                                   void* stream);
int bodyfit_forward_offsets_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                       const float* d_offsets, long long offsets_frame_stride, const float* d_grad_cloud,
                                       long long grad_cloud_row_floats, const double* d_grad_joints, double* d_grad_frame_params,
                                       double* d_grad_beta, float* d_grad_offsets, void* stream);
int bodyfit_forward_offsets_jvp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                       const float* d_offsets, long long offsets_frame_stride, int n_tangents,
                                       const double* d_tan_params, const double* d_tan_beta, double* d_tan_joints,
                                       float* d_tan_cloud, long long row_floats, void* stream);
/* Host-pointer forms, synchronous (cloud and gradient rows of 3 V floats; offsets and grad_offsets with the given stride: as in
 * the device form only the first 3 V floats of a grad_offsets row are written).  With offsets the forward is the two-launch one
 * of bodyfit_forward_offsets_device; with NULL offsets they are bodyfit_forward and bodyfit_forward_vjp.                     */
int bodyfit_forward_offsets(bodyfit_problem* p, const double* frame_params, const double* beta, const float* offsets,
                            long long offsets_frame_stride, double* joints, float* cloud);
int bodyfit_forward_offsets_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const float* offsets,
                                long long offsets_frame_stride, const float* grad_cloud, const double* grad_joints,
                                double* grad_frame_params, double* grad_beta, float* grad_offsets);

/* ---- the fitting objective as a differentiable function of (frame_params, beta) ----------------------------------------
 * Residual vector into caller memory: the sweep at (frame_params, beta) (without the mesh), then an asynchronous copy of the
 * problem's residuals [total_rows] (bodyfit_problem_layout row order) to d_residuals and, if d_gmm_comp [F] is not NULL, of the
 * GMM components.  keep_jacobian = 1 runs the Jacobian sweep, so that a following
 * bodyfit_residual_vjp_device(..., reuse_jacobian = 1) can skip its own sweep.  d_beta is required with the shape block.
 * Ordered like bodyfit_evaluate_device (it uses the problem's sweep buffers).                                              */
int bodyfit_residuals_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta, double* d_residuals,
                             int* d_gmm_comp, int keep_jacobian, void* stream);
/* Vector-Jacobian product of the WHOLE residual vector, given d_grad_residuals [total_rows] = dL/dr:
 *   d_grad_frame_params [F(+1)][7 + 3 (nJ - 1)] = (dr/dframe_params)^T g (the halo row of a temporal_halo problem receives the
 *   last temporal pair's -lambda g and nothing else), d_grad_beta [nS] (shared) or [F][nS] (beta_per_frame) = (dr/dbeta)^T g.
 * Row kinds: reprojection (the sweep's dense panel), pose prior (L2: beta_p I; GMM: beta_p s L_k^T, s = the mixture's
 * resid_scale, k = the frame's component at that sweep — the derivative of the residual as the sweep computes it; the
 * reference's analytic Jacobian of that block, which the solvers and bodyfit_evaluate_block reproduce, omits s; the constant
 * last row contributes nothing), shape prior (beta_s I), temporal (+-lambda I).
 * reuse_jacobian = 0: runs the Jacobian sweep at (frame_params, beta) first.  reuse_jacobian = 1: uses the Jacobian and GMM
 * components of the problem's last sweep, which the caller guarantees was at this point; BODYFIT_ERR_INVALID when the buffers
 * hold no current dense Jacobian (none since creation, or the last sweep was residual-only, or a solve or another sweep wrote
 * them since).  d_grad_beta is required when n_cols = 7 + 3 (nJ - 1) + nS, may be NULL otherwise (with use_shape = 0 only the
 * shape prior reaches it).  BODYFIT_ERR_INVALID also for NULL problem / frame_params / grad_residuals / grad_frame_params.
 * Asynchronous on `stream`, ordered like bodyfit_evaluate_device.  Deterministic: no atomics, fixed summation orders; a frame's
 * rows depend on that frame's rows of J and g only (bit-identical whatever F); a shared beta sums per-frame partials in a
 * fixed order.  The first call on a problem allocates (and, with a GMM prior, uploads) a little state of its own.           */
int bodyfit_residual_vjp_device(bodyfit_problem* p, const double* d_frame_params, const double* d_beta,
                                const double* d_grad_residuals, double* d_grad_frame_params, double* d_grad_beta,
                                int reuse_jacobian, void* stream);
/* Host-pointer form, synchronous, always re-sweeps. */
int bodyfit_residual_vjp(bodyfit_problem* p, const double* frame_params, const double* beta, const double* grad_residuals,
                         double* grad_frame_params, double* grad_beta);

/* ---- closest points between two per-frame point sets (the 3-D data term: scan / depth map / markers against the mesh) -----
 * A point set is f32 xyz rows on the device, organised per frame either uniformly (n_per_frame rows, frame_stride floats
 * between frames: bodyfit_device_views.cloud with its cloud_frame_stride, or a dense [F][n][3] array with stride 3 n) or
 * ragged (d_offset: a device int32 CSR [n_frames + 1] over one packed [N][3] array, the convention of kp_offset; frames may be
 * empty; d_offset[0] must be 0 and d_offset[n_frames] the set's row count: nothing checks it, since that would read the
 * offsets back).  The query set and the reference set may each be of either kind.                                          */
typedef struct bodyfit_pointset {
  const float* d_xyz;
  const int32_t* d_offset;   /* [n_frames + 1] CSR (ragged), or NULL: uniform                         */
  int n_per_frame;           /* uniform only                                                          */
  long long frame_stride;    /* uniform only, in floats, >= 3 n_per_frame                             */
} bodyfit_pointset;
typedef struct bodyfit_closest bodyfit_closest;   /* per-device workspace (partial minima, the groupings of the last searches) */
int bodyfit_closest_create(int device, bodyfit_closest** out);
void bodyfit_closest_destroy(bodyfit_closest* h);
/* For every query point p of frame f, over the reference points c_v of the same frame:
 *   d_index = argmin_v |p - c_v|^2, frame-local (-1 if the frame has no reference point, or every distance is NaN),
 *   d_dist2 = |p - c_index|^2 (+inf if none),
 * both packed in frame order: row d_offset[f] + i of a ragged query set, f n_per_frame + i of a uniform one.  The distance is
 * evaluated in f32 in the difference form (px - cx)^2 + (py - cy)^2 + (pz - cz)^2, so with D(v) the exact squared distance of
 * the two f32 points D(index) <= (1 + 2^-19) min_v D(v) and |dist2 - D(index)| <= 2^-20 D(index).  Among equal computed
 * distances the lowest index wins.  Deterministic, and a frame's outputs depend on that frame only (bit-identical whatever
 * n_frames).  n_query_total / n_ref_total: the row count of a ragged set (so that no call reads d_offset back to the host);
 * ignored for a uniform set.  prepare_vjp = 1 also groups the queries by the reference row they chose (integer work on the
 * index alone, about the cost of the gradient itself) and keeps that in the handle, so that
 * bodyfit_closest_points_vjp_device with this call's d_index is one launch; the handle keeps the groupings of its last four
 * such calls.  Asynchronous on `stream` (a hipStream_t as void*; NULL: the default stream); a call that has to
 * grow the handle's workspace synchronises the device once.  Calls on one handle share that workspace: order them (one stream,
 * or events).  n_frames == 0 or no query rows: a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / sets / outputs,
 * negative counts, frame_stride < 3 n_per_frame, 2^31 rows or more in a set.                                              */
int bodyfit_closest_points_device(bodyfit_closest* h, const bodyfit_pointset* query, const bodyfit_pointset* ref, int n_frames,
                                  long long n_query_total, long long n_ref_total, float* d_dist2, int32_t* d_index,
                                  int prepare_vjp, void* stream);
/* Reverse-mode gradient with the correspondence held fixed (the ICP / Chamfer gradient): given d_index (as above; -1 or an
 * index outside the frame: the query contributes nothing and gets a zero gradient) and d_grad_dist2 = dL/ddist2 (packed like
 * d_dist2),
 *   d_grad_query[i] = -2 g_i (c_index_i - p_i),        d_grad_ref[v] = sum over {i : index_i = v} of 2 g_i (c_v - p_i),
 * each in the layout of its point set (same d_offset / n_per_frame / frame_stride; every row of a frame is written, zeros
 * where no query maps; the padding between the frames of a uniform set is left untouched).  Either output may be NULL.  f32
 * throughout.  Deterministic: no float atomics; a reference row sums its queries in a fixed order that depends on that
 * frame's data only (ascending query row; a row that more than 64 queries chose: 64 interleaved ascending partial sums, then a
 * fixed tree), so a frame's gradients are bit-identical whatever n_frames and from run to run.  The grouping that dL/dref
 * needs is taken from the handle when d_index is the output pointer of one of its last four prepare_vjp searches over the same
 * sets and counts — the caller guarantees that the array has not been written since, and orders the two calls (one stream, or
 * events); any other d_index is grouped inside this call, at several launches more, with the same result bit for bit.
 * Asynchronous and ordered like bodyfit_closest_points_device.                                                             */
int bodyfit_closest_points_vjp_device(bodyfit_closest* h, const bodyfit_pointset* query, const bodyfit_pointset* ref,
                                      int n_frames, long long n_query_total, long long n_ref_total, const int32_t* d_index,
                                      const float* d_grad_dist2, float* d_grad_query, float* d_grad_ref, void* stream);

/* ---- closest point on the mesh SURFACE (the scan -> surface data term: a point on the posed surface costs nothing) ----------
 * A bodyfit_surface holds one topology on one device: the faces, the vertex -> (face, corner) CSR of the backward, and the
 * workspace of both calls (O(N + F n_faces): prepared triangle records, the splits' partial minima, the groupings of the last
 * four prepare_vjp searches, per-face gradient sums).  faces: host int32 [n_faces][3]; an id outside [0, n_verts) is
 * BODYFIT_ERR_INVALID; n_faces = 0 is accepted.  Degenerate faces (zero area, a repeated id, collinear corners) are legal: the
 * closest point is that of the segment or point the face collapses to.                                                        */
typedef struct bodyfit_surface bodyfit_surface;
int bodyfit_surface_create(int device, int n_verts, int n_faces, const int32_t* faces, bodyfit_surface** out);
void bodyfit_surface_destroy(bodyfit_surface* s);
/* For every query point p of frame f (query: a bodyfit_pointset of either kind), over the triangles
 * (verts[f][faces[t][0..2]]) of that frame (d_verts [F][n_verts][3] f32, verts_frame_stride floats between frames, >= 3 n_verts:
 * bodyfit_device_views.cloud is used in place): d_index the frame-local triangle, d_bary [N][3] the barycentric weights of the
 * closest point, d_dist2 the squared distance, packed in frame order like bodyfit_closest_points_device's outputs.
 * CONTRACT.  With c^ = sum_i b_i v_faces[index][i] and d^ = |p - c^| evaluated exactly from the f32 inputs, d* the exact minimum
 * distance from p to any triangle of the frame, h the longest edge of the returned triangle, u = 2^-24 and k = 32:
 *   b_i >= 0 and b_0 + b_1 + b_2 = 1 exactly (the weights are multiples of 2^-23);
 *   optimality   d^ <= d* + k u (d* + h);        consistency   |sqrt(d_dist2) - d^| <= k u (d^ + h).
 * The bound is on distances, never on which triangle wins: shared edges and vertices tie exactly.  Among equal COMPUTED
 * distances the lowest triangle index wins.
 * Derivation of k (k_closest_surface.hip).  A triangle T is evaluated in the orthonormal frame (u, w) of its longest edge AB,
 * prepared in f64 and rounded once, so a thin face loses nothing.  Write e = u (d_T + h_T) with d_T the exact distance of p to T
 * and h_T its longest edge; every quantity below is bounded by |p - A| <= d_T + h_T, and errors are absolute lengths.
 *  (1) what T's evaluation returns against T's exact closest point, E_T:
 *      X = ap . u and Y = ap . w: ap = p - A one rounding (|ap| u), a three-term dot three (3 |ap| u), the rounded unit vector
 *      one (|ap| u): 5 e per axis, 7.1 e for the in-plane point (x sqrt 2);
 *      the stored L, cx, t, one rounding each of lengths <= h_T: the 2-D triangle is off by at most 2 e;
 *      the projection onto an edge S + tau D: the dot (two terms of size |P - S| |D|) 2, the stored 1/|D|^2 1, the product 1,
 *      the point S + tau D 2: tau |D| is off by 6 u |P - S| <= 6 e;
 *      choosing among the candidates by their computed in-plane distances, each a sum of two squares of differences known to
 *      1.5 e: a wrong choice costs at most 3 e;
 *      the frame: u . w and |u|, |w| are off by u each, which tilts the 2-D picture by at most 2 e.      E_T <= 20.1 e.
 *  (2) the weights from (qx, qy): two divisions and one fused product (3 roundings of numbers <= 1, each moving c^ by u h_T),
 *      two roundings to 2^-23 (2^-24 each on a weight, the third weight takes both: 3 u h_T): 6 e.
 *  (3) dist2 against |p - (A + qx u + qy w)|^2: two fused steps per component on terms <= 3 (d_T + h_T), 6 e per component,
 *      10.4 e for the vector (x sqrt 3); the sum of squares and the root 2 e; u L against B - A and w t against C's offset 2 e:
 *      with (2), consistency 20.4 e, stated as k = 32.
 *  Optimality: the winner W has the smallest computed distance, so its point is bounded through the exactly closest triangle
 *  T*: d^_W <= d* + E_T* + 6 e_W.  With W = T* that is 26.1 e, stated as k = 32.  With W != T* the evaluation error of T* scales
 *  with ITS longest edge, so what holds without condition is the bound with h = max(h_W, h_T*); the form above, in the returned
 *  triangle's h alone, holds whenever h_T* <= 1.29 h_W (20.1 of the units ride on h_T*, 32 - 6 = 26 are available), as between
 *  the neighbouring faces of a mesh, where such ties occur.  No f32 evaluation can promise more: a point d* from a large face
 *  and d* + delta from a small one, delta below the rounding of p - A at the large face's size, cannot be told apart.  The
 *  tests assert the stricter form, in the returned triangle's h, for every query of their face soups.
 * A conservative cull skips a triangle when the computed squared distance to the midpoint of AB exceeds (s + R)^2, with
 * s = sqrt(best) (1 + 2^-12) and R = (1 + 2^-12) x the radius of the sphere about that midpoint (R >= L / 2).  Its margin in
 * distance is at least 2^-12 (sqrt(best) + R) >= 2^-13 L = 2048 u L.  Against it: the midpoint distance in the expanded form
 * |ap|^2 - L X + L^2 / 4 carries at most 6 u (|ap| + L)^2; far away (|ap| > 4 L) that is a relative 10 u, nothing beside
 * 2^-12; nearer, 150 u L^2, which over twice the distance (>= R >= L / 2) is 150 u L; and the pair's own evaluation error,
 * k u (d + h) with d <= 5 L and h = L, is 192 u L: 342 u L < 2048 u L.  So a culled triangle's COMPUTED distance is above the
 * running best; it could neither win nor tie, and the cull never changes an output bit.
 * Deterministic: bit-identical from run to run, whatever the split of the face range and whatever n_frames (a frame's outputs
 * depend on that frame only).
 * A NaN / Inf query, or a triangle with a non-finite corner, never wins; a query without a finite candidate (also n_faces = 0)
 * gets d_index = -1, d_dist2 = +inf, d_bary = 0.  prepare_vjp = 1 also groups the queries by the face they chose and keeps
 * that in the handle, as for bodyfit_closest_points_device.  Asynchronous on `stream`; a call that has to grow the handle's
 * workspace synchronises the device once; calls on one handle share the workspace: order them.  n_frames == 0 or no query
 * rows: a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / set / outputs, negative counts, a stride below 3 n_verts.    */
int bodyfit_closest_surface_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_verts,
                                   long long verts_frame_stride, int n_frames, long long n_query_total, float* d_dist2,
                                   int32_t* d_index, float* d_bary, int prepare_vjp, void* stream);
/* The ORIENTED search: bodyfit_closest_surface_device over the normal-compatible triangles only.  Query row i carries a
 * direction m_i (d_query_normals: [N][3] f32, packed in frame order, row-aligned with d_dist2 whatever the layout of the query
 * set; the scan's own normal, or for a depth map the direction towards the sensor).  A triangle is a candidate for the row iff
 * it has an area and its face normal n, in the orientation of `faces` ((v1 - v0) x (v2 - v0) normalised), has n . m_i >= min_cos.
 * m is used as given: the caller passes unit vectors; a zero vector has n . m = 0.  Among the candidates everything is as above:
 * the same evaluation, cull, tie-break, outputs and conventions; a row without a candidate gets -1, +inf, 0.  The gate is
 * piecewise constant in the vertices, so the gradient at the fixed (index, bary) is unchanged: the backward is
 * bodyfit_closest_surface_vjp_device on the returned arrays, and a grouping prepared here (prepare_vjp) is found by it exactly as
 * one of the unoriented search.  A NaN in m_i: row i has no candidate; a NaN min_cos: no row has.
 * CONTRACT.  With u = 2^-24, k_n = 16 and tau_i = k_n u |m_i|, let n_t be the exact unit normal of the f32 corners of face t,
 * "with area" the rule of the prepared record (height over the longest edge L above 2^-40 L and above 1e-30), and
 *   strict_i = {t with area : n_t . m_i >= min_cos + tau_i},      loose_i = {t with area : n_t . m_i >= min_cos - tau_i}.
 *   (1) the returned triangle is in loose_i, or d_index = -1;
 *   (2) if strict_i is not empty, d_index != -1 and d^ <= d*_strict + k u (d*_strict + h), k = 32, with d^ and h as above and
 *       d*_strict the exact minimum distance from p_i to the triangles of strict_i;
 *   (3) if loose_i is empty, d_index = -1;
 *   (4) the properties of b_i and the consistency bound hold as above;
 *   (5) deterministic and frame-independent as above: a face on the threshold may fall either way, but always the same way.
 * Derivation of k_n (k_closest_surface.hip), in units of u, for |m| = 1 (everything scales with |m|).  The record holds the
 * orthonormal in-plane frame u, w of the longest edge, formed in f64 and rounded once: every component is off by at most 1
 * (|component| <= 1).  The corner rotation of the record is cyclic, so u x w is the face normal in the orientation of `faces`:
 * (B - A) x (C - A) = L t (u x w).  n = u x w is formed per component as fma(a, b, -(c d)): the two products of perturbed inputs
 * carry 4, the two roundings (the product c d, the fused result; both numbers <= 1) 2: 6 per component.  s = n . m is a
 * three-term fma chain: the components' 6 weighted by |m_c|, at most 6 sqrt 3 = 10.4, and its own three roundings of partial
 * sums <= |m|, 3.  Total 13.4 against the f64 normal of the record, stated as k_n = 16; the f64 frame itself is exact to 2^-52
 * over the relative height, nothing beside u for any face a scan can tell from a segment.  The gate only REMOVES candidates
 * between the cull and the evaluation, so the cull argument above stands unchanged: a culled triangle's computed distance is
 * above a running best that is the distance of an admitted candidate.
 * Checks, workspace, asynchrony and the no-op rules are those of bodyfit_closest_surface_device; also BODYFIT_ERR_INVALID for a
 * NULL d_query_normals when there are query rows.                                                                            */
int bodyfit_closest_surface_oriented_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_query_normals,
                                            float min_cos, const float* d_verts, long long verts_frame_stride, int n_frames,
                                            long long n_query_total, float* d_dist2, int32_t* d_index, float* d_bary,
                                            int prepare_vjp, void* stream);
/* Reverse-mode gradient at the fixed correspondence (d_index and d_bary held; by the envelope theorem the true gradient of the
 * squared distance almost everywhere, since the weights minimise): with c^_i = sum_a b_ia v_faces[index_i][a],
 *   d_grad_query[i] = 2 g_i (p_i - c^_i),     d_grad_verts[f][v] = sum over (i, a) with faces[index_i][a] = v of -2 g_i b_ia (p_i - c^_i),
 * d_grad_query in the layout of the query set, d_grad_verts in that of d_verts (every vertex row of every frame is written,
 * zeros where nothing maps; the padding behind a frame is left untouched).  Either output may be NULL.  d_index = -1 or out of
 * range contributes nothing.  f32; p - c^ is formed as (p - v0) - b1 (v1 - v0) - b2 (v2 - v0).  Deterministic: no float
 * atomics; per face the queries that chose it in ascending order (more than 64: 64 interleaved ascending partial sums, then a
 * fixed tree), then per vertex its incident (face, corner) sums in ascending order.  The grouping is taken from the handle
 * when d_index is the output of one of its last four prepare_vjp searches over the same set and counts, else built inside this
 * call, with the same result bit for bit.  Asynchronous and ordered like bodyfit_closest_surface_device.                     */
int bodyfit_closest_surface_vjp_device(bodyfit_surface* s, const bodyfit_pointset* query, const float* d_verts,
                                       long long verts_frame_stride, int n_frames, long long n_query_total, const int32_t* d_index,
                                       const float* d_bary, const float* d_grad_dist2, float* d_grad_query, float* d_grad_verts,
                                       void* stream);
/* The VJP of "barycentric x direction" ROWS (k_cs_rows_vjp_faces, k_cs_rows_vjp_verts): row i of frame f (the rows' frame
 * structure is that of `rows`, a point set as above of which only d_offset / n_per_frame are used; d_xyz is not read, but must
 * not be NULL) carries d_index[i] = t_i, d_bary[i] = b_i [3] f32, d_coef[i] f32 and d_dir[i] = m_i [3] f32, and
 *   d_gverts[f][v] = sum over the rows i of frame f and the corners a with faces[t_i][a] = v of  coef_i b_ia m_i,
 * [F][n_verts][3] f32, gverts_frame_stride floats between frames (>= 3 n_verts; the padding is left untouched).  Every vertex of
 * every frame is written, 0 where nothing lands; a row with t_i = -1 or out of range contributes nothing and its other entries are
 * never read; the vertices themselves are not an argument.  This is dL/dverts of the depth rows of
 * bodyfit_raster_depth_rows_device with coef = dL/dz, and the right-hand side of any point-to-plane row (coef = -w_i r_i, m the
 * unit normal).
 * Two scatter-free stages, as bodyfit_closest_surface_vjp_device: per (frame, face) the nine sums S[a][c] = sum_i coef_i b_ia m_ic
 * over the rows that chose the face, in ascending row order, in f64 (a face more than 64 rows chose: 64 interleaved ascending
 * partial sums, then a fixed tree); then per (frame, vertex) its incident (face, corner) sums in ascending order through the
 * handle's vertex -> corner table, in f64, rounded ONCE to f32.  Integer atomics only inside the grouping; no float atomics.  The
 * result is bit-identical from run to run, whatever n_frames (a frame's gradient depends on that frame's rows only), and whether
 * the grouping by face was kept or rebuilt: it is taken from the handle when d_index is the output of one of its last four
 * prepare_vjp searches over the same set and counts, else built inside this call.  The handle cannot see another writer: a
 * d_index that anything but such a search wrote (the depth rows kernel, the caller) must not be a buffer whose kept grouping is
 * still in the handle, or must have a search's invalidating write in between; a buffer no search of this handle wrote is always safe.
 * CONTRACT, u = 2^-24: with G* the exact sum above and T the same sum of the terms' absolute values, both evaluated exactly from
 * the f32 rows,   |d_gverts - G*| <= 2 u T   per component.
 * The count, eps = 2^-53 = 2^-29 u: coef_i b_ia is exact in f64 (48 significant bits), its product with m_ic rounds once; a term
 * then passes at most max(64, N / 64 + 6) additions in its face's sum, N < 2^31 rows: 2^25 + 6, and at most as many as its vertex
 * has incident corners in the second; every addition costs eps times the absolute sum so far, at most eps T.  Together (2^25 + 8
 * + valence) eps T = (2^-4 + 2^-29 valence) u T, and the one rounding to f32 adds u |G^| <= u (1 + 2^-3) T: below 2 u T for every
 * vertex with fewer than 2^28 incident corners, that is for every mesh of fewer than 89 million faces whatever its shape.
 * Workspace: 72 bytes per (frame, face), shared with the surface VJP's.  Asynchronous on `stream`, ordered like the other calls
 * on the handle.  n_frames == 0 or n_verts == 0: a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / set / d_gverts, with rows
 * a NULL d_index / d_bary / d_coef / d_dir or set's d_xyz, negative counts, gverts_frame_stride < 3 n_verts, 2^31 - 4096 or more
 * rows, (frame, face) or (frame, vertex) pairs.                                                                               */
int bodyfit_surface_rows_vjp_device(bodyfit_surface* s, const bodyfit_pointset* rows, int n_frames, long long n_rows_total,
                                    const int32_t* d_index, const float* d_bary, const float* d_coef, const float* d_dir,
                                    float* d_gverts, long long gverts_frame_stride, void* stream);
/* The WINDING NUMBER of the frame's posed mesh about every query point (k_winding.hip): is the point inside the body?  For a query
 * p and a triangle t with corners v0, v1, v2 in the orientation of `faces`, a = v0 - p, b = v1 - p, c = v2 - p (van Oosterom and
 * Strackee):    num = a . (b x c),    den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|,    Omega_t(p) = 2 atan2(num, den),
 *   d_winding[i] = w(p_i) = (1 / 4 pi) sum over the frame's faces of Omega_t(p_i),      packed in frame order like d_dist2.
 * atan2(0, 0) = 0: a face that has p as a corner contributes 0, and so does a face without an area.  For a closed, outward oriented
 * mesh w is the number of times the surface encloses p (0 outside, 1 inside, 2 inside two overlapping parts); for an open mesh it
 * is the generalised winding number and varies smoothly; reversing every face reverses the sign.
 * d_skip_vertex (int32 [N], packed like d_winding, or NULL): row i leaves out the faces that have the id d_skip_vertex[i] >= 0
 * among their three corner ids (a comparison of ids, not of positions); -1 skips none.  The VERTEX query is the uniform set
 * {d_verts, n_verts, verts_frame_stride} with the ids 0 .. n_verts - 1 in every frame: then w_i = k_i + (the interior solid angle
 * of the cone of faces about vertex i) / 4 pi, k_i the number of OTHER sheets of the surface that enclose the vertex and the cone's
 * share strictly between 0 and 1, so vertex i lies inside another part of the body iff w_i > 1.
 * A frame with a non-finite corner in any face gives NaN for every query row of that frame (whatever the rows skip); a non-finite
 * query row gives NaN; other frames and rows are untouched.  n_faces = 0 gives 0.
 * CONTRACT.  With u = 2^-24, l_t = |a||b||c| and z_t = den + i num, all exact from the f32 inputs, w* the exact value, and every
 * distance from a query to a corner between 2^-40 and 2^40 or exactly 0 (no intermediate overflows or underflows),
 *   |d_winding[i] - w*_i| <= B_i = (u / 2 pi) sum over the counted faces of (k l_t / |z_t| + k_s),        k = 64, k_s = 16.
 * |z_t| = 0 with l_t > 0 happens exactly when p lies on an edge of t or in its plane across an edge at the angle where Omega
 * jumps: there the bound is infinite and only a finite result is promised.  A face with l_t = 0 (p is a corner) has num = den = 0
 * exactly, in f32 as in exact arithmetic, and counts k_s alone.  OUTSIDE that range of distances the result is UNDEFINED, and may be
 * a finite number: finite corners far enough away overflow the products of three lengths, the arctangent then yields a NaN, and
 * the integer sum takes that NaN's bits for a number.  Only non-finite INPUTS are promised to give NaN.
 * Derivation (k_winding.hip; first order in u, the stated constants leave a tenth for the rest).  theta_t = atan2(num, den) is
 * half the solid angle and w = sum theta_t / 2 pi, so an error e_t of theta_t moves w by e_t / 2 pi.  An error (dn, dd) of
 * (num, den) turns theta by at most (|dn| + |dd|) / |z|.
 *  num: a, b, c are one subtraction each (u per component).  A component of b x c is fma(x, y, -(z w)): the four inputs 2 u, the
 *   product's rounding 1, the fused result's 1, each of at most |b||c|: 4 u |b||c| per component, 6.93 for the vector.  a . n is a
 *   three-term fma chain: a's own u, n's 6.93, three roundings of partial sums <= |a||n|: |dn| <= 10.93 u l.
 *  den: |a| = sqrt of a three-term chain of squares: the inputs 2 u, three roundings, halved by the root, the root's own rounding:
 *   3.5 u; the product of three lengths 3 x 3.5 + 2 = 12.5 u l.  A dot a . b: inputs 2 u, roundings 3 u, of |a||b|; times a length
 *   8.5 u l, three of them 25.5 u l.  The three fused additions round partial sums of at most 2 l, 3 l and 4 l: 9 u l.
 *   |dd| <= 47 u l.                                                           Together 57.93 u l / |z|, stated as k = 64.
 *  the arctangent, absolute, in u: mx, mn the larger and smaller of |num|, |den|; above tan(pi / 8) the argument is (mn - mx) / (mn +
 *   mx): three roundings on |t| <= 0.4143, atan' <= 1: 1.25.  The polynomial t + t z P(z) (four coefficients) is within 0.14 of atan
 *   there (tests/test_winding.py checks that figure of the coefficients), its evaluation costs 0.2 on the cubic part and 0.4 for
 *   the last fused step.  + pi / 4: the constant 0.4, the sum 0.8.  pi / 2 - r: 0.73 and 1.57.  pi - r: 1.47 and 3.14.  Together 10.1.
 *  the sum: theta is rounded to a multiple of 2^-32 (0.002) and added as an integer, EXACTLY; sum 2^-32 / 2 pi in f64 and one rounding
 *   to f32, u |w| <= u n / 2 for n counted faces, that is pi in the units of k_s.        10.1 + 0.002 + 3.15 = 13.3, stated as k_s = 16.
 * tests/winding_ref.py computes w* and B_i in f64 and restates the kernel's arithmetic in f32.  On a unit sphere of 2,560 faces
 * next to a second one, B_i stays below 8e-4 at every vertex while w_i keeps 0.41 away from the threshold 1.
 * Deterministic, and more: the sum is exact, so a row's bits do not depend on the split of the face range, on the wave a face fell
 * to, on n_frames or on the frame's place in the batch: a frame's result is a function of that frame's data and counts only.  No
 * atomics.  Query sets of either kind.  Workspace: with few query rows the face range is split and 8 bytes per (split, row) are
 * kept; nothing per (frame, face).  Checks, asynchrony, ordering and the no-op rules are those of bodyfit_closest_surface_device
 * (n_frames == 0 or no query rows: a successful no-op; BODYFIT_ERR_INVALID: NULL handle / set / d_winding, negative counts, a
 * stride below 3 n_verts).  NOT differentiable: w is piecewise constant off the surface.                                      */
int bodyfit_surface_winding_device(bodyfit_surface* s, const bodyfit_pointset* query, const int32_t* d_skip_vertex,
                                   const float* d_verts, long long verts_frame_stride, int n_frames, long long n_query_total,
                                   float* d_winding, void* stream);
/* Area-weighted VERTEX NORMALS of the posed mesh (k_winding.hip):  n_i = normalise(sum over the faces t that hold vertex i of
 * (v1 - v0) x (v2 - v0)), every face once and oriented as in `faces`; d_normals [F][n_verts][3] f32, dense.  A vertex without a
 * face, with a zero sum or with a non-finite corner in one of its faces gets 0.  One thread per (frame, vertex) adds the faces in
 * ascending order through the handle's vertex -> corner table in f64 (the differences of f32 corners are exact, the products are
 * not fused, so a face that repeats a corner adds an exact zero), normalises in f64 and rounds ONCE:
 *   |d_normals - n*| <= u + 2^-50 c_i per component,   c_i = sum |N_t| / |sum N_t| (how much the faces about the vertex cancel),
 * u = 2^-24: one rounding of a number <= 1, and the f64 roundings of at most eight operations per face, amplified by c_i.
 * Deterministic (no atomics; torch's index_add_ is not), frame-independent.  NOT differentiable: the oriented search uses the
 * normals as a gate, which is piecewise constant.  Asynchronous on `stream`.  n_frames == 0 or n_verts == 0: a successful no-op.
 * BODYFIT_ERR_INVALID: NULL handle / d_verts / d_normals, a negative n_frames, a stride below 3 n_verts.                      */
int bodyfit_surface_vertex_normals_device(bodyfit_surface* s, const float* d_verts, long long verts_frame_stride, int n_frames,
                                          float* d_normals, void* stream);
/* THE VERTEX NORMALS' ADJOINT (k_vn_h, k_vn_vjp, k_light.hip): for an upstream d_grad_normals f32 [F][n_verts][3] = dL/dn, dense,
 * d_grad_verts f32 [n_verts][3] per frame, grad_frame_stride floats between frames (>= 3 n_verts; its own stride) = dL/dverts through
 * bodyfit_surface_vertex_normals_device at the f32 vertices; every element of the [n_verts][3] blocks is written.
 * DEFINITION.  s_i = sum_{t holds i} N_t, N_t = (v1 - v0) x (v2 - v0), n_i = s_i / |s_i|;
 *   h_i = (g_i - n_i (n_i . g_i)) / |s_i|, and h_i = 0 where the forward wrote 0 (no face, a zero sum, a non-finite corner);
 *   a_t = (h_i0 + h_i1) + h_i2;       dL/dv_{t,a} += (v_{t,a+1} - v_{t,a+2}) x a_t, corner indices cyclic.
 * A face that repeats a vertex id contributes nothing (its N_t is identically 0), and neither does a face whose a_t is exactly 0 (so
 * a non-finite vertex, whose faces all have h = 0 at their corners, spreads nothing and receives 0).  The upstream is plain IEEE.
 * Two passes.  The first, one thread per (frame, vertex), forms s_i by the FORWARD's arithmetic (the same faces in the same order by
 * the same f64 operations: n_i is the forward's before its store) and stores h_i as f64 in the handle's workspace.  The second,
 * one thread per (frame, vertex), gathers over the vertex's entries of the handle's vertex -> corner table in ascending order in
 * f64 (the edge, a difference of f32 corners, is exact; products and sums unfused) and rounds ONCE.  No atomics, frame-independent,
 * bit-identical from run to run.
 * CONTRACT, with u = 2^-24, eps = 2^-53, k_v = 128, c_i of the forward, and per face A_t = sum over its corners a of c_ia |g_ia| /
 * |s_ia| (>= |a_t|):       |gv^ - gv*| <= u |gv*| + k_v eps sum over the vertex's faces of |v_{t,a+1} - v_{t,a+2}| A_t   per component.
 * Derivation.  The forward's contract puts n_i within 8 eps c_i of exact and |s_i| within 8 eps c_i relative; h_i: a dot product
 * (5 eps), a product, a difference, a quotient: |dh_i| <= (2 x 8 c_i + 8 c_i + 6) eps |g_i| / |s_i| <= 32 c_i eps |g_i| / |s_i|.
 * a_t: the three dh and two sums: 34 eps A_t.  A component of the cross product: two products and a difference of magnitudes <=
 * |e| |a_t| each: 2 x (34 + 2) eps |e| A_t; the sums over the faces one eps per face more on the running sum (valence <= 50 in
 * practice; 128 covers it).  The store's u.
 * Workspace: 24 bytes per (frame, vertex), kept by the handle (a growth synchronises the device once).  Otherwise asynchronous on
 * `stream`.  n_frames == 0 or n_verts == 0: a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / d_verts / d_grad_normals /
 * d_grad_verts, a negative n_frames, a stride below 3 n_verts.                                                                 */
int bodyfit_surface_vertex_normals_vjp_device(bodyfit_surface* s, const float* d_verts, long long verts_frame_stride, int n_frames,
                                              const float* d_grad_normals, float* d_grad_verts, long long grad_frame_stride,
                                              void* stream);
/* The uniform mesh LAPLACIAN of per-vertex fields (k_offsets.hip), the smoothness operator of an offset field's regulariser:
 * field k is [n_verts][3] f32 at d_field + k field_stride (>= 3 n_verts), d_out [n_fields][n_verts][3] f32, dense, not d_field.
 * With n_i the number of faces that hold vertex i (a face that repeats i counted once) and a, b the face's other two corner
 * POSITIONS (taken from i's first position in it):
 *   l_i = x_i - (1 / 2 n_i) sum_{t holds i} (x_a + x_b),   l_i = 0 when n_i = 0   (an interior vertex: x_i - mean of its ring).
 * transpose = 1 applies the exact transpose:  (L^T r)_u = [n_u > 0] r_u - sum_{t holds u} sum_{other corners v} r_v / (2 n_v)
 * (for a vertex without a face both its row and its column of L are zero, so both directions give it 0).
 * One thread per (field, vertex) gathers over the vertex's entries of the handle's vertex -> corner table in ascending order, in
 * f64, and rounds once: |d_out - exact| <= 2^-24 |exact| + 2^-48 sum |x| over the vertex and its ring.  No atomics (torch's
 * index_add_ is not deterministic, and not needed), field-independent.  Asynchronous on `stream`.  n_fields == 0 or n_verts == 0:
 * a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / d_field / d_out, d_out == d_field, a negative n_fields, a stride
 * below 3 n_verts.                                                                                                          */
int bodyfit_surface_laplacian_device(bodyfit_surface* s, const float* d_field, long long field_stride, int n_fields,
                                     int transpose, float* d_out, void* stream);
/* The Gauss-Newton NORMAL EQUATIONS of a scan term at a fixed correspondence, per frame, without ever holding a per-row Jacobian
 * (k_surface_gram.hip).  Row i of frame f (packed like d_dist2) carries d_index[i] = t_i, d_bary[i] = b_i, optionally a weight
 * w_i (d_weight [N] f32; NULL: 1) and a unit direction d_i (d_direction [N][3] f32; NULL: point-to-point).  d_jac is the dense
 * Jacobian of the frame's vertices in the layout of bodyfit_forward_jvp_device's d_tan_cloud: [F][P][row_floats] f32, P =
 * n_tangents, tangent p of frame f at d_jac + f jac_frame_stride + p row_floats, its first 3 V floats J_f[p][v][0..2] (row_floats
 * >= 3 V; what lies behind the 3 V floats of a row is never read and may hold anything, NaN included).
 * CONTRACT.  With A_i[:, p] = sum_a b_ia J_f[p][faces[t_i][a]][0..2], the 3-vector by which tangent p moves the row's surface point,
 *   d_H[f][p][q] = sum_i w_i (A_i[:, p] . A_i[:, q])                        without d_direction (point-to-point),
 *   d_H[f][p][q] = sum_i w_i (d_i . A_i[:, p]) (d_i . A_i[:, q])            with it (point-to-plane),
 * over the rows i of frame f with 0 <= t_i < n_faces, [F][P][P] f64, the full symmetric panel; and, with d_rhs [F][V][3] f32
 * (rhs_frame_stride floats between frames, >= 3 V), d_g[f][p] = sum_v J_f[p][v] . rhs_f[v], [F][P] f64 (d_g NULL: not computed;
 * d_g needs d_rhs).  These are J^T W J and J^T rhs of the cost 1/2 sum_i w_i |r_i|^2 when rhs = dcost/dverts.  A row with t_i = -1
 * or out of range, or with w_i = 0, contributes nothing; a frame without rows gets exact zeros.
 * How: sum_i w_i A_i^T D_i A_i = J^T W J with W the 3 V x 3 V matrix of the per-face moments M_t[a][c] = sum_{i -> t} w_i b_ia b_ic
 * D_i (D_i = I or d_i d_i^T), non-zero on the mesh's vertices and edges only: moments per face, the sparse mix Y = W J, and the
 * dense contraction H = J . Y^T on the matrix pipe (bf16 hi / lo split of both operands, hi.hi + hi.lo + lo.hi, f32
 * accumulation over slices of 256 floats of the contracted index, the slices' partial panels summed in f64).
 * PRECISION.  With H* the exact value of the formula above on the f32 inputs, and H^ the same sum with every factor replaced by
 * its absolute value and the dot products expanded, H^[p][q] = sum_i |w_i| sum_{a,c,x,y} |b_ia b_ic D_i[x][y] J[p][v_a][x] J[q][v_c][y]|
 * (D_i[x][y] = [x = y] or d_ix d_iy),
 *   |d_H - H*| <= eps H^ elementwise, eps = 2^-12;      |d_g - g*| <= eps_g g^, eps_g = 2^-32, g^ = sum_k |J[p][k] rhs[k]|.
 * Derivation, in units of u = 2^-24.  Moments: products and sums in f64 (each term carries at most 6 roundings of 2^-53, a sum of
 * n terms n more: below 2^-28 u for any n < 2^21), rounded once to f32: 1.  Y: f64 sums of f32 x f32 products (exact), at most
 * 2^-20 u, rounded once to f32: 1.  The split: x = hi + lo + r with hi the bf16 nearest x (8 significant bits: |x - hi| <= 2^-8
 * |x|) and lo the bf16 nearest x - hi, so |lo| <= 2^-8 |x| and |r| <= 2^-16 |x|; the three products that are formed miss lo.lo
 * and the terms in r: 2^-16 + 2 x 2^-16 (1 + 2^-7) < 3.02 x 2^-16 = 773.2 of a product J Y, stated as 776.  bf16 x bf16 is exact
 * in f32.  The f32 accumulation of one partial panel entry is a chain of 3 x 256 terms whose absolute values sum to at most
 * (1 + 2^-6) |J||Y|; with at most 2 per addition (the matrix pipe's sums are not promised to round to nearest) that is
 * 2 x 768 x 1.016 = 1561.  The f64 fold of the partial panels: 2^-29 per slice, nothing.  Together 1 + 1 + 776 + 1561 = 2339
 * < 4096 = 2^-12 / u, first-order terms only; the second-order ones are below 1.  (Measured on random inputs: 2e-5 H^ at the
 * worst, the split's share.)  g: products of two f32 are exact in f64, the sum of n = 3 V terms carries n 2^-53, stated as 2^-32
 * (n < 2^21).
 * DETERMINISM.  H is exactly symmetric (the triangle p >= q is computed, the other is its copy).  No float atomics; per face the
 * rows in ascending order under the 64-partial rule of bodyfit_closest_surface_vjp_device, then fixed orders over a vertex's
 * incident corners, the contracted index and the slices: a frame's panel depends on that frame only, bit-identical whatever
 * n_frames, from run to run, and whether the grouping was kept or rebuilt.
 * The grouping by face is taken from the handle when d_index is the output of one of its last four prepare_vjp searches over the
 * same set and counts, else built inside the call, as for bodyfit_closest_surface_vjp_device (query->d_xyz is not read, but must
 * not be NULL).  The vertex -> corner table is the handle's, built in bodyfit_surface_create.  Workspace: the moments, Y and the
 * partial panels of SIXTEEN frames at a time (the groups follow one another on the stream): per frame of a group
 * P 3 V 4 bytes of Y, 24 (144 with directions) bytes per face and 4 KiB per (tile pair, slice), 11 MB at SMPL size with
 * P = 86, whatever n_frames; growing it synchronises the device once, as for the searches.  Asynchronous on `stream`,
 * ordered like the other calls on the handle.  n_frames == 0: a successful no-op.  BODYFIT_ERR_INVALID: NULL handle / set /
 * d_index / d_bary / d_jac / d_H, n_tangents < 1 or > 4096, row_floats < 3 V, jac_frame_stride < n_tangents row_floats,
 * rhs_frame_stride < 3 V, d_g without d_rhs, negative counts, a (n_tangents, V) whose partial panels pass 2^31 bytes per frame. */
int bodyfit_surface_gram_device(bodyfit_surface* s, const bodyfit_pointset* query, int n_frames, long long n_query_total,
                                const int32_t* d_index, const float* d_bary, const float* d_weight, const float* d_direction,
                                const float* d_jac, int n_tangents, long long row_floats, long long jac_frame_stride,
                                const float* d_rhs, long long rhs_frame_stride, double* d_H, double* d_g, void* stream);

/* The post-solve write-back of a whole solve on the device: for every frame
 *   r[0] <- R(rootAA) r[0]  (left-multiplied, so it compounds over repeated solves),  p <- rootT,
 *   r[j] <- R(jointAA[j]),  Avatar::update()  (the Sim3 scale is dropped),
 * as OptimizeMultiFrame / OptimizePose*Reprojection do per frame on the host (include/MultiFrameBA.h:154-174,
 * include/Sim3BA.h:481-505), followed by mean_pixel_error (include/Utils.h:102-115) of the frame's FK-joint
 * keypoints against the updated joints (0 for a frame without any).
 * Outputs, each optional: R0_out [F][9] row-major, joints [F][nJ][3], cloud [F][V][3] (needs want_mesh; the posed
 * cloud also stays resident, see bodyfit_problem_views), mean_px [F].                                      */
int bodyfit_writeback_batch(bodyfit_problem* p, const double* frame_params, const double* beta, double* R0_out,
                            double* joints, float* cloud, double* mean_px);

/* include/Utils.h:102-115 on the joints of bodyfit_forward (no Sim3 scale: pass scale = 1). */
double bodyfit_mean_pixel_error(int n_kp, const int* jid, const double* uv, const double* joints,
                                double fx, double fy, double cx, double cy);

/* ---- outer loop (what the reference hands to ceres::Solve) ------------------------------------
 * Ceres-like trust-region Levenberg-Marquardt over one bodyfit_problem (see host_solver.cpp for the
 * restated algorithm).  Every evaluation is one device sweep; the linear solve is a block-tridiagonal
 * Cholesky with a Schur complement on the shared shape block: on the device by block cyclic reduction over the
 * frames (k_window_lm.hip), for short windows on the host (host_solver.cpp).
 *   frame_params [F][76] in/out, beta [nS] or [F][nS] in/out (NULL when n_cols == 76)
 *   param_constant [76] flags or NULL: 1 = SetParameterBlockConstant (include/Sim3BA.h:608-611)
 *   independent_frames 1: every frame is its own problem with its own LM state (3dba_single: frames
 *   are fitted independently, src/main_single_frame.cpp:192); 0: one problem over all frames
 *   (OptimizeMultiFrame).  summaries: one per problem (F or 1).                                  */
typedef struct bodyfit_fit_options {
  int max_iters;            /* ceres::Solver::Options::max_num_iterations */
  double scale_lo, scale_hi;/* SetParameterLowerBound / UpperBound on the scale: 0.3, 3.0 */
  int verbose;
  int solver;               /* 0 auto: independent frames iterate on the device (k_lm_batched); a shared-beta window
                               of >= 12 frames iterates on the device too (k_window_lm: block cyclic reduction over the
                               frames), shorter ones on the host; 1 force the host loop; 2 force the device loop for
                               independent frames; 3 force the device loop for a shared-beta window */
} bodyfit_fit_options;
typedef struct bodyfit_fit_summary {
  int iterations;           /* LM iterations (successful + unsuccessful) */
  int termination;          /* 0 convergence, 1 iteration limit, 2 failure */
  int usable;               /* Summary::IsSolutionUsable() */
  int n_successful, n_unsuccessful;
  int n_sweeps;             /* device evaluations the solve needed.  Device window LM: 1 + one per iteration (the sweep at a
                               candidate also leaves its Jacobian); host loop and the batched LM in its four-launch form: 1 + one
                               per iteration + one per accepted step */
  double initial_cost, final_cost;
  int n_sweeps_issued;      /* ... and the sweeps actually launched: the device window LM runs up to three iterations ahead of
                               the host's status reads (they find the solve terminated and change nothing); 0 = same as n_sweeps */
} bodyfit_fit_summary;
int bodyfit_solve(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                  int independent_frames, const bodyfit_fit_options* options, bodyfit_fit_summary* summaries,
                  int n_summaries);

/* ---- one window sharded over several GPUs (frames = the data-parallel axis of OptimizeMultiFrame) -----------
 * One process per GPU.  Rank r creates a bodyfit_problem over ITS contiguous frames (temporal_halo = 1 on every rank but
 * the last: the temporal pair that leaves the shard is evaluated by the shard it leaves; beta_shape > 0 on exactly one
 * rank) and calls bodyfit_solve_sharded with a communicator.  The LM state is replicated by construction (every rank
 * takes the same decisions from the same reduced scalars); the linear solve is substructured: cyclic reduction of the
 * local chain down to its two end frames, an all-gather of those 2 N interface blocks, the interface system solved by
 * every rank, local back-substitution.  The shared-shape terms [H_bb, g_beta] cross the ranks ONCE per LM iteration.
 * Per LM iteration the ranks exchange THREE all-gathers (the 2 N interface blocks with the beta terms riding on them, 225 KB
 * per rank; the beta Schur partials, 110 doubles; six scalars) and every rank sums the gathered partials in rank order, so the
 * decisions are identical everywhere without a broadcast.  Two transports:
 *   bodyfit_solve_sharded        the caller's callback on HOST buffers (device -> host -> callback -> device; torch.distributed
 *                                "gloo" in the tests, MPI in a C++ host).  Only `allgather` is called; `allreduce` may be NULL.
 *   bodyfit_solve_sharded_rccl   RCCL on the solve's device buffers and stream (ncclAllGather over xGMI): no host staging and no
 *                                stream synchronisation between the host's status reads (every fourth iteration).
 * Both callbacks / RCCL calls must be entered by every rank of the communicator the same number of times.  Failures:
 *   - a rank whose own device work fails (the first sweep, or a kernel launch / HIP call inside an LM iteration) does NOT leave on its own: it marks
 *     its scalars, keeps taking part in that iteration's exchanges, and the decision kernel ends the solve on EVERY rank in the
 *     same iteration; all ranks then return an error (the failing one its own, the others "another rank reported a device
 *     failure") after the same number of exchanges — nobody is left waiting;
 *   - a failure of the transport itself (a callback that returns non-zero, an RCCL error) returns at once on the rank that saw
 *     it; its peers may be waiting in that exchange: bodyfit_set_exchange_timeout (below) bounds that wait inside the library,
 *     whatever timeout the process group / RCCL has of its own.
 *   frame_params [F_local (+1 halo row)][76] in/out: the halo row is refreshed from the neighbour by the solve. */
/* A bound, in seconds, on every exchange and every status read of this problem's sharded solves (0, the default: none).  With it
 * a transport failure cannot strand the peers of the rank that saw it: a host callback that has not returned within the bound
 * (bodyfit_solve_sharded; the callback then runs on a helper thread, which is left behind with its own copies of the buffers) or a
 * stream that has not drained (an RCCL collective its peer never entered) ends the solve with BODYFIT_ERR_HIP on that rank too.
 * The problem's solve stream is not usable after such a return.  An abandoned callback keeps running on its helper thread: its
 * `ctx` must stay valid until it returns; and bodyfit_problem_destroy waits for the device, so with the RCCL transport abort or
 * destroy the communicator first (a collective that will never complete would hold that wait too).  Choose the bound well above
 * one LM iteration (milliseconds); it is a liveness guard, not a pacing device. */
int bodyfit_set_exchange_timeout(bodyfit_problem* p, double seconds);
typedef struct bodyfit_comm {
  int rank, size;
  void* ctx;
  int (*allreduce)(void* ctx, double* buf, int n, int op /* 0 sum, 1 max */);            /* unused since round 3; may be NULL */
  int (*allgather)(void* ctx, const double* send, double* recv /* [size][n] */, int n);
} bodyfit_comm;
int bodyfit_solve_sharded(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                          const bodyfit_comm* comm, const bodyfit_fit_options* options, bodyfit_fit_summary* summary);

/* RCCL communicator of the sharded solve.  librccl is bound at run time (dlopen), so libbodyfit.so has no link-time dependency
 * on it.  Either let the library create the communicator — rank 0 obtains the 128-byte id (ncclGetUniqueId) and ships it to the
 * other ranks by any host channel, every rank then calls bodyfit_rccl_create (ncclCommInitRank, collective) — or hand in an
 * ncclComm_t the application already has (bodyfit_rccl_wrap; not destroyed by bodyfit_rccl_destroy).                       */
typedef struct bodyfit_rccl bodyfit_rccl;
int bodyfit_rccl_unique_id(unsigned char* id128);
int bodyfit_rccl_create(const unsigned char* id128, int rank, int size, int device, bodyfit_rccl** out);
int bodyfit_rccl_wrap(void* nccl_comm, int rank, int size, bodyfit_rccl** out);
void bodyfit_rccl_destroy(bodyfit_rccl* c);
int bodyfit_solve_sharded_rccl(bodyfit_problem* p, double* frame_params, double* beta, const unsigned char* param_constant,
                               bodyfit_rccl* comm, const bodyfit_fit_options* options, bodyfit_fit_summary* summary);
/* The evaluation path's one collective (include/MultiFrameBA.h:64-68 — the shared shape block — summed over the
 * shards): ncclAllReduce(sum, f64) of the 66 doubles [cost | g_beta | upper H_bb], in place on the device buffer, on `stream`:
 * behind bodyfit_evaluate_device + bodyfit_reduce_shared_device on the same stream it needs no host synchronisation.    */
int bodyfit_allreduce_shared_rccl(bodyfit_rccl* comm, double* d_buf66, void* stream);
/* ranks of the communicator and this process's rank, as RCCL reports them (ncclCommCount, ncclCommUserRank) */
int bodyfit_rccl_count(bodyfit_rccl* comm, int* n_ranks, int* rank);
/* Measurement aid for boxes with ONE GPU: this problem's following sharded solves through a one-rank communicator run as rank
 * `rank` of `n_ranks` IDENTICAL shards — the local chain reduced with its ends pinned, the interface chain of 2 n_ranks frames,
 * every all-gather issued (on the one-rank communicator; a small kernel then fills the other n_ranks - 1 gathered slots with
 * copies of this shard's), sums over n_ranks slots, the neighbours' boundary steps.  The problem must be shaped like that rank's
 * shard (temporal_halo = 1 unless rank == n_ranks - 1).  What it times is ONE rank's critical path at that geometry with the
 * transport's latency at its lower bound; the fitted numbers belong to a window of n_ranks copies of the shard, not to the
 * caller's sequence.  n_ranks <= 1 switches it off.  bench.py's c5_strong.shard_proxy uses it. */
int bodyfit_set_shard_proxy(bodyfit_problem* p, int n_ranks, int rank);
/* all-gathers issued by the problem's last sharded solve (tests assert the number of exchanges per iteration) */
long bodyfit_last_exchange_count(const bodyfit_problem* p);

/* Normal equations of the reprojection blocks, built on the device (window solvers: bodyfit_solve's host loop,
 * the numpy cross-check tests/sharded_lm_check.py): evaluate at (frame_params, beta) and return the residual vector [total_rows], the
 * GMM components [F] (may be NULL) and, per frame, the lower triangle of J^T rho' J over its n_cols columns with the
 * gradient J^T rho' r in row n_cols, as a [F][87][88] row-major panel (HuberLoss weights rho' applied per keypoint,
 * include/MultiFrameBA.h:64,102).  Prior and temporal blocks have constant Jacobians and are left to the caller.
 * Needs <= 32 keypoints per frame.                                                                        */
int bodyfit_frame_normals(bodyfit_problem* p, const double* frame_params, const double* beta, double* residuals,
                          int* gmm_comp, double* normals);

/* ---- mesh overlay ------------------------------------------------------------------------
 * smpl::render::renderSMPLMesh(cloud, faces, img, fx, fy, cx, cy, fill, backface_cull, wireframe) of
 * include/RenderSMPLMesh.h:16-110, batched over frames with the posed vertices and the 8-bit BGR images
 * resident on the device: project (:36-46), per-face cull / flat shade / painter depth / integer corners
 * (:50-88), far-to-near order (:91-92; ties by face index, the reference's std::sort leaves them unspecified)
 * and cv::fillConvexPoly(..., LINE_AA) per triangle in that order (:95-104).  The result is, pixel for pixel,
 * what drawing the triangles one after the other gives.  wireframe != 0 adds cv::polylines in gray 40 after each
 * triangle's fill (:106-109; the reference's callers never enable it: src/main_single_frame.cpp:274,
 * src/main_multi_frame.cpp:210,223); fill == 0 and wireframe == 0 draws nothing, as there.
 *   faces [n_faces][3] vertex ids (ark::AvatarModel::mesh columns, src/main_single_frame.cpp:185-188)
 *   cloud: x, y, z per vertex (the memory order of the reference's 3xN column-major `cloud`), camera
 *   coordinates; cloud_is_f64 0: float (bodyfit_device_views.cloud of a write-back), 1: double
 *   images: n_frames images of height x width x 3 bytes, row_stride / frame_stride in bytes, modified in place
 *   (the reference draws into a clone of the video frame)                                                    */
typedef struct bodyfit_overlay bodyfit_overlay;
typedef struct bodyfit_overlay_desc {
  int device;
  int n_vertices, n_faces;
  const int32_t* faces;
  int width, height;
  int max_frames;
} bodyfit_overlay_desc;
int bodyfit_overlay_create(const bodyfit_overlay_desc* desc, bodyfit_overlay** out);
void bodyfit_overlay_destroy(bodyfit_overlay* ov);
/* device pointers; asynchronous on `stream` except for one 8-byte read-back that sizes the tile lists */
int bodyfit_overlay_render_device(bodyfit_overlay* ov, const void* d_cloud, int cloud_is_f64,
                                  size_t cloud_frame_stride_elems, int n_frames, uint8_t* d_images,
                                  size_t row_stride, size_t frame_stride, double fx, double fy, double cx,
                                  double cy, int fill, int backface_cull, int wireframe, void* stream);
/* host pointers (upload, render, download): the one-call form of the reference function */
int bodyfit_overlay_render(bodyfit_overlay* ov, const void* cloud, int cloud_is_f64, size_t cloud_frame_stride_elems,
                           int n_frames, uint8_t* images, size_t row_stride, size_t frame_stride, double fx,
                           double fy, double cx, double cy, int fill, int backface_cull, int wireframe);
/* draw list of `frame` from the latest render (far to near): face ids [n], corners [n][6] = x0 y0 x1 y1 x2 y2,
 * gray levels [n]; each array may be NULL; returns the count in *n_items                                   */
int bodyfit_overlay_drawlist(bodyfit_overlay* ov, int frame, int* n_items, int32_t* face, int32_t* corners,
                             int32_t* gray);
/* average launch durations (ms) of the overlay kernels of the latest render_device call, by HIP events:
 * [0] faces, [1] sort + rank, [2] binning (count, scan, fill), [3] tiles                                  */
int bodyfit_overlay_last_timing(bodyfit_overlay* ov, float ms[4]);

/* ---- depth render and visibility (k_raster.hip): what one calibrated camera sees of the posed mesh ---------------------------
 * A bodyfit_raster holds one topology (faces: host int32 [n_faces][3], ids in [0, n_verts), else BODYFIT_ERR_INVALID; n_faces =
 * 0 is accepted) and one image size (1 .. 16384 each way) on one device, and the workspace of its calls, which grows on demand
 * (96 bytes per (frame, face), 12 per (frame, tile of 32 x 8 pixels), 4 per (face, tile) pair; 8 per pixel of the frames of a
 * distance transform), and 12 bytes per face of edge neighbours for the antialiasing calls.                                                                                                     */
typedef struct bodyfit_raster bodyfit_raster;
int bodyfit_raster_create(int device, int n_verts, int n_faces, const int32_t* faces, int width, int height,
                          bodyfit_raster** out);
void bodyfit_raster_destroy(bodyfit_raster* r);
/* The z-buffer of n_frames posed meshes (d_verts [F][n_verts][3] f32, verts_frame_stride floats between frames, >= 3 n_verts:
 * bodyfit_device_views.cloud is used in place): per frame d_depth f32 [H][W] (+inf where empty), d_face int32 [H][W] (-1 where
 * empty) and, unless NULL, d_bary f32 [H][W][3] (0 where empty), dense, frame after frame.  Every pixel of every frame is
 * written: nothing depends on what the outputs held.
 * DEFINITION, evaluated exactly from the f32 vertices and the f64 intrinsics (fx, fy > 0).  Corner a of a face projects to
 * (u_a, v_a) = (fx X_a / Z_a + cx, fy Y_a / Z_a + cy), the convention of the keypoint residual; pixel (row i, column j) is the
 * sample s = (j, i).  With A = (p1 - p0) x (p2 - p0) the doubled signed area of the projected face (x: the 2-D cross product),
 * face t is DRAWN iff its nine coordinates are finite, every Z_a >= z_near, and A != 0; with cull_backfaces also A < 0.  A < 0 is
 * a front face: A = fx fy (n . v0) / (Z0 Z1 Z2) with n = (v1 - v0) x (v2 - v0) the normal in the orientation of `faces`, so A < 0
 * iff n points to the camera, the orientation (counter-clockwise seen from outside, y down) in which the overlay's backface_cull
 * keeps a face.  (The overlay tests n_z < 0, the sign of n . v0 for a face on the optical axis; the two differ only on faces
 * seen nearly edge-on away from the image centre, where n_z and n . v0 have different signs.)  A face with a corner in front
 * of z_near is dropped WHOLE: there is no clipping.  The screen-space barycentrics of s are lambda_a = (p_b - s) x (p_c - s) / A
 * (b, c the two corners after a); a drawn face covers s iff all three are >= 0 (edges inclusive); its depth there is the
 * perspective-correct z = 1 / sum_a lambda_a / Z_a.  The pixel gets the covering face of least z, ties to the lowest face id,
 * and that face's lambda in d_bary.
 * CONTRACT, with u = 2^-24, k_e = 2, k_z = 2 and per face P_t = max_a max(|u_a|, |v_a|) + max(W, H) + max(|cx|, |cy|) (a bound
 * on every corner, and on every corner - sample), Q_t = P_t^2 / |A_t|, R_t = max_a Z_a / min_a Z_a,
 *   tau_t = k_e u (1 + 2^-22 Q_t),        c_t = 2^-19 Q_t R_t.
 * Call a drawn face SURELY COVERING at s when min_a lambda_a >= tau_t and SURELY MISSING when min_a lambda_a < -tau_t.  Then at
 * every pixel, with t^ the returned face and z^ the returned depth:
 *   (a) t^ is not surely missing (and has finite corners at or behind z_near, and with cull_backfaces A <= 2^-46 P_t^2);
 *   (b) |z^ - z(t^, s)| <= (k_z + c_t^) u z^, z(t^, s) evaluated at the lambda clamped to the triangle (negative ones to 0,
 *       the rest rescaled to sum 1);
 *   (c) z^ <= (1 + (k_z + c_t) u) z(t, s) for every surely covering t;
 *   (d) the pixel is empty only if no face surely covers it;
 *   (e) the returned weights are >= 0, within tau_t^ of the exact lambda of t^, and sum to 1 within 2 tau_t^.
 * For a face of a body mesh in an HD image Q_t is about 2^18 and R_t about 1: tau_t = 2.1 u and c_t < 1, so (b) is 3 u z^.  The
 * terms in Q_t are the price of a sliver: no evaluation from rounded projections can place a sample against an edge of a face
 * whose area is lost in P_t^2.  Q_t = infinity (A = 0 to the last bit) makes (a), (c), (d) empty statements, as they must be.
 * Derivation (k_raster.hip; eps = 2^-53 = 2^-29 u).  Everything that decides is f64.  u_a: the quotient, the product and the sum
 * round once each, 3 eps P.  A corner - sample difference d: one more, 4 eps P, |d| <= P.  An edge function E = d1 d2 - d3 d4
 * with the two products rounded separately (never fused: a sample exactly on an edge gives exactly 0, and the two faces of a
 * shared edge compute E and -E): three roundings of numbers <= 2 P^2, 4 eps P^2, and four factors off by 4 eps P against
 * partners <= P, 16: 20 eps P^2.  A, from corner differences <= 2 P known to 8 eps P: 64 + 16 = 80 eps P^2.  lambda = E (1 / A):
 * two more roundings; for |lambda| <= 1 the error is at most 100 eps Q + 2 eps.  In units of u that is 100 x 2^-29 Q <= 2^-22 Q:
 * the decision lambda >= 0 is right outside a band of 2^-22 Q u, and the f32 rounding of a returned weight adds at most u: tau
 * with k_e = 1, stated as 2 for the second-order terms.  The integer bounding box in front of the evaluation (ceil / floor of
 * the computed corners) removes only samples outside the exact triangle or within 3 eps P of its box, far inside the band.
 * Depth: 1 / z^ = sum lambda^_a (1 / Z_a) from the computed weights (all >= 0), against the clamped exact ones at most
 * 3 x 100 eps Q apart each: relative to the sum that is 9 x 100 eps Q R = 7.1 x 2^-22 Q R u <= c_t u; the sum's own roundings
 * are a few eps; the reciprocal and its conversion to f32 round once each: 1 u + eps, stated as k_z = 2.  The order is decided
 * on the f64 1 / z before that conversion, which gives (c); among equal 1 / z the lowest face id wins, whatever the order in
 * which the tile lists were filled, so the result is bit-identical from run to run and a frame's images depend on that frame
 * only (bit-identical whatever n_frames).  A NaN or infinite vertex only removes its faces.
 * Shape: a face kernel prepares one 96-byte record per (frame, face); the faces are binned to 32 x 8 tiles by bounding box (a
 * count, an allocation, a fill; integer atomics); one workgroup per (frame, tile) stages its records through LDS and keeps a
 * pixel's (1 / z, face) in registers; plain stores.  No float atomics.
 * Asynchronous on `stream` except for ONE 8-byte read-back that sizes the tile lists (the only host synchronisation, as in
 * bodyfit_overlay_render_device; none when n_faces = 0) and for a call that has to grow the workspace.  Calls on one handle
 * share the workspace: order them.  n_frames == 0: a successful no-op; n_faces == 0: every pixel empty, no face kernel runs.
 * BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames, z_near <= 0 or NaN, fx or fy <= 0 or a non-finite
 * intrinsic, and with frames to write: NULL d_depth / d_face, NULL d_verts (n_faces > 0), a stride below 3 n_verts, 2^31 or
 * more (frame, face) or (frame, tile) pairs.                                                                                 */
int bodyfit_raster_render_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                 double fx, double fy, double cx, double cy, float z_near, int cull_backfaces,
                                 float* d_depth, int32_t* d_face, float* d_bary /* may be NULL */, void* stream);
/* Visibility from a face-id image (d_face int32 [n_frames][H][W], as rendered; a value outside [0, n_faces) is empty):
 * d_face_visible u8 [n_frames][n_faces], 1 iff the face owns at least one pixel of its frame, else 0; d_vert_visible u8
 * [n_frames][n_verts], 1 iff the vertex is a corner of such a face.  Exact: integer work, no tolerance.  Either output may be
 * NULL (both: a no-op).  Asynchronous on `stream`, no host synchronisation.  BODYFIT_ERR_INVALID: NULL handle, negative
 * n_frames, NULL d_face with something to write.                                                                             */
int bodyfit_raster_visibility_device(bodyfit_raster* r, const int32_t* d_face, int n_frames,
                                     uint8_t* d_face_visible /* may be NULL */, uint8_t* d_vert_visible /* may be NULL */,
                                     void* stream);
/* DEPTH ROWS: the projective depth residual's rows at the correspondence a render already holds (k_rs_depth_rows, k_raster_rows.hip).
 * A row is a pixel of a frame; its face is what d_face_image (int32 [n_frames][H][W], as rendered by this handle's topology and
 * size; a value outside [0, n_faces) is empty) holds there.  d_pixel int32 [N]: the linear index i W + j inside the row's frame;
 * d_offset int32 [n_frames + 1]: the rows of frame f are offset[f] .. offset[f + 1] - 1 (offset[0] = 0, offset[n_frames] = N, the
 * ragged convention of the closest searches), or NULL: N / n_frames rows per frame.  Both NULL: every pixel of every frame in
 * image order, N = n_frames H W.  Outputs, packed per row: d_index int32 [N] the face or -1, d_z f32 [N], d_bary f32 [N][3],
 * d_dir f32 [N][3]; any of the last three may be NULL.  Every row is written, whatever the outputs held.
 * DEFINITION, from the f32 corners v0, v1, v2 of the face (order of `faces`) and the f64 intrinsics, for pixel (row i, column j):
 *   ray d = ((j - cx) / fx, (i - cy) / fy, 1),   n = (v1 - v0) x (v2 - v0),   D = n . d,
 *   z = (n . v0) / D          the z of the ray-plane intersection x = z d; wherever the pixel lies in the face this is the
 *                             render's perspective-correct 1 / sum_a lambda_a / Z_a,
 *   beta_a = n . ((v_b - x) x (v_c - x)) / (n . n)   (b, c the corners after a): the OBJECT-space barycentrics of x, sum 1; not
 *                             the screen-space lambda of bodyfit_raster_render_device,
 *   m = n / D                 which does not depend on the orientation of `faces`.
 * At the fixed face dz/dv_a = beta_a m^T: the plane moves with its corners through n . (beta_a delta) only, the change of n
 * multiplies x - p = 0 for the point p = sum beta_a v_a = x.  So a depth row is a point-to-plane row of
 * bodyfit_surface_gram_device (weights beta on the three corners, direction m / |m|, weight w |m|^2) and its gradient a row of
 * bodyfit_surface_rows_vjp_device (coef = dL/dz).  1 / (|m| |d|) is the cosine between the face normal and the ray.
 * A row is VOID when its pixel index is outside [0, H W), its pixel is empty, a corner is not finite, or the f64 evaluation
 * below gives n = 0 or D = 0 (an exact n = 0 gives it whenever the corner differences are exact in f64, that is for coordinates
 * within 2^29 of one another: the two products of a component are then rounded from equal numbers).  A void row gets index -1,
 * z = +inf, beta = 0, m = 0.  z may be negative (a plane met behind the camera): that is not void.  beta is returned as
 * computed, NOT renormalised and NOT clamped: a pixel in the render's coverage band (lambda within tau_t of 0) has a slightly
 * negative weight, and a row whose face does not contain the pixel has weights outside [0, 1].
 * CONTRACT, with u = 2^-24, k = 2 and per non-void row x = z d exact and
 *   P = the largest magnitude among the nine corner coordinates and the three of x,
 *   L = the largest magnitude among the coordinate differences corner - corner and corner - x (the face's extent when the
 *       pixel lies in it),
 *   Q = P L / |n|,   rho = max(1, P / |x|),   c = |D| / (|n| |d|)  (the cosine above),
 *   kappa = 2^-21 rho Q / c,        kappa_b = 2^-18 rho Q^2 / c:
 *   |z^ - z| <= (k + kappa) u |z|,    |m^_c - m_c| <= (k + kappa) u |m|,    |beta^_a - beta_a| <= (k + kappa_b) u max(1, |beta|),
 * |m| the Euclidean and |beta| the largest-magnitude norm (|beta| <= 1 wherever the pixel lies in the face).
 * Q is the analogue of the render's Q_t: the face's |n| against the product of where it lies and how far it reaches.  With f32
 * corners the squared corner coordinates themselves never enter: a difference of two f32 is formed in f64 with a rounding
 * relative to the difference (exactly, for coordinates within 2^29 of one another), so n is lost against L^2, not P^2; P enters
 * once through n . v0 (rho, c: a plane that passes near the camera, a grazing ray) and once through x in beta.  For a 2 cm face
 * of a body at 3 m Q is about 300: kappa = 2^-13, kappa_b = 2^-1.5, so the three bounds are 2 u, 2 u and 2.4 u.  A row the
 * evaluation voids although n and D are not 0 has kappa >= 2^24 (shown below): the bound it would have exceeds z itself.
 * Derivation (eps = 2^-53 = 2^-29 u; every operation f64, products and sums separately rounded, never fused; S = L^2 / |n|,
 * 1/3 <= S <= 2 Q because |n| <= |e1| |e2| <= 3 L^2 and L <= 2 P).  e = v_b - v_0: |e_c| <= L, off by eps L.  A component of n:
 * two products <= L^2 (2 eps L^2), their difference <= 2 L^2 (2 eps L^2), four factors off by eps L against partners <= L
 * (4 eps L^2): 8 eps L^2, |dn| <= 14 eps L^2 = 14 eps S |n|.  d: a difference and a quotient, 2 eps |d|.  D = (n_x d_x + n_y d_y)
 * + n_z: |dn| |d|, 2 eps |n| |d| from d, two products and two sums of numbers <= sqrt 3 |n| |d| (7 eps): dD <= eps |n| |d| (14 S +
 * 9).  N0 = n . v0 with |v0| <= sqrt 3 P: 24.3 eps S |n| P from dn and 5.2 eps |n| P from three products and two sums.  z = N0 / D
 * with |N0| = |z| |D| and |D| = c |n| |d|, one more rounding:
 *   dz / |z| <= eps [rho (24.3 S + 5.2) + 14 S + 9] / c + eps <= 84 eps rho S / c <= 168 eps rho Q / c = 2^-21.6 rho Q / c u,
 * stated as kappa; the store rounds once more: 1 u, stated as k = 2 for the terms of second order.  m_c = n_c / D:
 * |dn| / |n| + dD / |D| + eps <= 58 eps S / c <= 116 eps Q / c relative to |m|, inside kappa, and the store's u |m_c|.  beta: x^ =
 * z^ d^ is off by |x| (dz / |z| + 3 eps) <= sqrt 3 P 93 eps rho S / c; it enters p = v_b - x and q = v_c - x alike, so p x q moves
 * by dx x (v_b - v_c) and n . (p x q) / (n . n) by at most sqrt 3 L |dx| / |n| <= 279 eps rho Q S / c.  Apart from that p and q are
 * off by eps L, p x q like n by 14 eps L^2, |p x q| <= 3 L^2; n . (p x q): 42 eps L^4 + 14 eps |n| L^2 + 15.6 eps |n| L^2; n . n and
 * its reciprocal and the product: (28 S + 5) eps relative, |beta| <= 3 S.  Together
 *   dbeta <= eps S [126 S + 44.6 + 279 rho Q / c] <= 1598 eps rho Q^2 / c = 2^-18.4 rho Q^2 / c u,
 * stated as kappa_b, and the store's u |beta_a|, k = 2.  A void by n^ = 0 needs |n| <= |dn|, S >= 2^53 / 14; by
 * D^ = 0, c <= eps (14 S + 9): either way Q / c >= 2^53 / 82 and kappa >= 2^25.
 * AGAINST THE RENDER.  Where d_face_image is this handle's render of the same vertices and intrinsics, item (b) of its contract
 * bounds the rendered depth against z(t^, s) at the clamped lambda, which is the z above when the pixel lies in the face (min
 * lambda >= 0) and at most 9 tau_t R_t z away from it inside the coverage band.  So at every covered pixel
 *   |z_row - z_rendered| <= (k + kappa) u |z| + (k_z + c_t) u z_rendered + [min lambda < 0] 9 tau_t R_t z:
 * the sum of the two contracts.
 * One thread per row, a gather of the face's 36 bytes of corners; plain stores, no atomics.  Asynchronous on `stream`, no host
 * synchronisation, no workspace.  n_frames == 0 or N == 0: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): NULL
 * handle, negative n_frames or n_rows, fx or fy <= 0 or a non-finite intrinsic, d_offset without d_pixel, without d_pixel an
 * n_rows other than n_frames H W, a uniform d_pixel whose n_rows n_frames does not divide, 2^31 - 4096 rows or more, and with
 * rows to write: NULL d_face_image / d_index, NULL d_verts (n_faces > 0), a stride below 3 n_verts.                             */
int bodyfit_raster_depth_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                     double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                     const int32_t* d_pixel /* may be NULL */, const int32_t* d_offset /* may be NULL */,
                                     long long n_rows, int32_t* d_index, float* d_z /* may be NULL */,
                                     float* d_bary /* may be NULL */, float* d_dir /* may be NULL */, void* stream);
/* INTERPOLATION ROWS: the gradient of vertex attributes interpolated over a face, and of the ray-plane depth, in the face's three
 * corners, at the correspondence a render already holds (k_rs_interp_rows, k_raster_rows.hip).  What bodyfit_raster_shade_device lacks:
 * how a pixel's colour changes when its face moves under the fixed pixel ray.  Rows, d_face_image, d_pixel, d_offset and n_rows are
 * exactly those of bodyfit_raster_depth_rows_device.  d_attr f32 rows of n_channels floats per vertex, attr_frame_stride floats
 * between frames (0: shared by the frames, else >= n_channels n_verts), as in bodyfit_raster_shade_device; d_grad_image f32
 * [n_frames][H][W][n_channels] = G = dL/dimage and d_grad_z f32 [n_frames][H][W] = g_z = dL/dz or NULL, both DENSE images: a row
 * reads them at its own (frame, pixel), so nothing is gathered before the call.  n_channels in 0 .. 4; 0 (d_attr and d_grad_image
 * may be NULL) is the depth-only case, which needs d_grad_z.  Outputs, packed per row: d_index int32 [N] the face or -1, d_bary f32
 * [N][3], d_dir f32 [N][3], d_value f32 [N][n_channels]; any of the last three may be NULL.  Every row is written, whatever the
 * outputs held.
 * DEFINITION.  With d, n, D, z, x, beta and m of bodyfit_raster_depth_rows_device and A_a the attribute row of corner a, the
 * interpolated value is I_ch = sum_a beta_a A_a,ch (d_value).  At the fixed face and the fixed ray let
 *   g_a = n x (v_c - v_b) / (n . n)   (b, c the corners after a): the in-plane gradient of beta_a, g_a . n = 0, sum_a g_a = 0,
 *   h_a = g_a - (g_a . d / D) n = g_a - (g_a . d) m:   h_a . d = 0, sum_a h_a = 0, |h_a|^2 = |g_a|^2 + (g_a . d)^2 |m|^2.
 * Moving corner c by delta moves the plane's point on the ray by (beta_c m . delta) d (the depth rows' dz/dv_c = beta_c m^T), and a
 * point that stays in the plane keeps sum_b beta_b (v_b - x) = 0: differentiating, with g_a the derivative of beta_a in the point,
 * gives dbeta_a/dv_c = -beta_c h_a^T.  So for upstream gradients G_ch and g_z
 *   dL/dv_c = beta_c dir,   dir = g_z m - sum_a s_a h_a,   s_a = sum_ch G_ch A_a,ch:
 * ONE row of bodyfit_surface_rows_vjp_device per pixel whatever n_channels (index = the face, bary = beta, coef = 1, direction =
 * dir).  dir . d = g_z; three equal s_a (a face of one colour) give dir = g_z m exactly.
 * VOID rows are the depth rows': index -1, beta = 0, dir = 0, value = 0.  Attributes and upstream gradients are plain IEEE: a NaN
 * or an infinity there gives a non-finite dir (and value) and does NOT void the row; those of a void row are never read.
 * CONTRACT, with u = 2^-24, k_i = 2, P, L, Q, rho, c and kappa_b of the depth rows, and per non-void row
 *   sigma_a = sum_ch |G_ch A_a,ch|,   T = |g_z| |m| + sum_a |s_a| |h_a|,   T_1 = |g_z| |m| + sum_a sigma_a |h_a|   (T <= T_1, equal
 *       for n_channels <= 1 and wherever the channels of a corner do not cancel in s_a),
 *   kappa_d = 2^-19 rho Q / c,   V_ch = sum_a |beta_a A_a,ch|,   A_ch = sum_a |A_a,ch|:
 *   |dir^_c - dir_c| <= k_i u T + kappa_d u T_1,     |value^_ch - I_ch| <= k_i u V_ch + kappa_b u max(1, |beta|) A_ch,
 * and index and beta are the depth rows', bit for bit (the same operations in the same order).  The bound is relative to T, not
 * to |dir|: the three h_a sum to 0, so |dir| can be far below T and no evaluation from rounded corners keeps a bound relative to
 * it.  The first term is the store's rounding, the second the f64 evaluation under the face's conditioning: for the 2 cm face of
 * a body at 3 m of the depth rows' example kappa_d = 2^-11 and the bound is 2 u T.
 * Evaluation order, chosen so that equal s_a cancel EXACTLY: s_a = ((G_0 A_a0 + G_1 A_a1) + G_2 A_a2) + G_3 A_a3 (a product of
 * two f32 is exact in f64), the DIFFERENCES p = s_1 - s_0 and q = s_2 - s_0 against s_0, E = q e1 - p e2 with the depth rows' e1 =
 * v1 - v0 and e2 = v2 - v0 (E = sum_a s_a (v_c - v_b)), w = (n x E) (1 / (n . n)) = sum_a s_a g_a, k = (w_x d_x + w_y d_y) + w_z,
 * a = w - k m = sum_a s_a h_a, dir = g_z m - a; value_ch = (beta_0 A_0ch + beta_1 A_1ch) + beta_2 A_2ch from the unrounded beta.
 * Derivation (eps = 2^-53 = 2^-29 u; f64, unfused; S = L^2 / |n| <= 2 Q and the depth rows' |dn| <= 14 eps S |n|, 1 / (n . n) to
 * (28 S + 5) eps, m_c to 58 eps S / c |m|).  s_a: at most three sums, 3 eps sigma_a.  p, q: one rounding more, |p| + |q| <= 2 Sigma
 * with Sigma = sigma_0 + sigma_1 + sigma_2.  A component of E, two products of factors off by eps L and their difference:
 * L (dp + dq + 5 eps (|p| + |q|)) <= 16 eps L Sigma, |dE| <= 28 eps L Sigma.  Every edge has |n| <= |v_c - v_b| sqrt 3 L (the area
 * is an edge times a height, and a height is below another edge), so L / |n| <= sqrt 3 S |g_a| for EVERY a and L Sigma / |n| <=
 * sqrt 3 S T_g with T_g = sum_a sigma_a |g_a| <= T_1: the price of the differences (a term in sigma_0 |e1|, which the face's own
 * T_g need not hold) is one factor S, which kappa_d carries anyway.  w, |w| = |E| / |n| <= T_g: the cross product and the
 * product with the reciprocal 12 eps, dn 14 eps S, the reciprocal 28 eps S, dE 49 eps S: |dw| <= eps (91 S + 12) T_g.  k: |dk| <=
 * (|dw| + 8 eps |w|) |d|, and |m| |d| = 1 / c.  k m_c: |k| |m| <= sum_a |s_a| |h_a| (since |g_a . d| |m| <= |h_a|), so dk |m| + |k|
 * dm_c + eps |k m_c| <= eps ((91 S + 20) / c T_g + (58 S / c + 1) T_1).  a_c = w_c - k m_c rounds once more, 2 eps T_1.  Together
 *   |da_c| <= eps T_1 (240 S + 35) / c <= 345 eps S T_1 / c <= 690 eps Q T_1 / c = 2^-19.6 Q / c u T_1;
 * g_z m_c is off by |g_z| |m| 116 eps Q / c, inside the same kappa_d (rho >= 1 is kept so that one number serves both parts; it
 * multiplies nothing in a).  The last difference and the store: eps and u of |dir^_c| <= T (1 + ...), stated as k_i = 2.  value:
 * beta^_a before its store is within kappa_b u max(1, |beta|) of beta_a (the depth rows' derivation), three products and two
 * sums 3 eps V_ch, the store u: k_i = 2.  A row voided although n and D are not 0 has kappa >= 2^24, as a depth row.
 * AGAINST THE SHADE.  Where d_face_image and the shade's d_bary are this handle's render of the same vertices and intrinsics and
 * the shade does not void the pixel, the shade's image is sum_a w_a(lambda^) A_a within its k_s u T_ch, w_a(lambda) = (lambda_a /
 * Z_a) / sum_b (lambda_b / Z_b).  For the EXACT screen-space lambda of the pixel in the face, w_a(lambda) = beta_a (both are the
 * barycentrics of the ray's point in the plane, inside the face or not), and item (e) of the render's contract keeps lambda^
 * within tau_t of lambda: each lambda_a / Z_a moves by tau_t / Z_a, their sum by at most 3 tau_t R_t of itself, so |w_a(lambda^) -
 * beta_a| <= 5 tau_t R_t (for tau_t R_t <= 1/16: 4 to first order).  So at every such pixel
 *   |value_row_ch - image_shade_ch| <= k_i u V_ch + kappa_b u max(1, |beta|) A_ch + k_s u T_ch + 5 tau_t R_t A_ch:
 * the two contracts and the render's summed.
 * One thread per row: a gather of the face's 36 bytes of corners and 12 n_channels bytes of attributes, the upstream gradients
 * streamed at the row's pixel; plain stores, no atomics, no workspace: bit-identical from run to run, and a frame's rows depend on
 * that frame only.  Asynchronous on `stream`, no host synchronisation.  n_frames == 0 or N == 0: a successful no-op.
 * BODYFIT_ERR_INVALID (nothing is launched): every case of bodyfit_raster_depth_rows_device (NULL handle, negative n_frames or
 * n_rows, fx or fy <= 0 or a non-finite intrinsic, d_offset without d_pixel, without d_pixel an n_rows other than n_frames H W, a
 * uniform d_pixel whose n_rows n_frames does not divide, 2^31 - 4096 rows or more, and with rows to write: NULL d_face_image /
 * d_index, NULL d_verts (n_faces > 0), a stride below 3 n_verts), n_channels outside 0 .. 4, and with rows to write: NULL d_attr
 * / d_grad_image with n_channels > 0, a non-zero attribute stride below n_channels n_verts, n_channels == 0 without d_grad_z.     */
int bodyfit_raster_interp_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                      double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                      const int32_t* d_pixel /* may be NULL */, const int32_t* d_offset /* may be NULL */,
                                      long long n_rows, const float* d_attr, long long attr_frame_stride, int n_channels,
                                      const float* d_grad_image, const float* d_grad_z /* may be NULL */, int32_t* d_index,
                                      float* d_bary /* may be NULL */, float* d_dir /* may be NULL */,
                                      float* d_value /* may be NULL */, void* stream);
/* INTERPOLATION ROWS WITH PER-CORNER ATTRIBUTES (k_rs_interp_rows<C, true>, the same kernel template with one more compile-time
 * switch): bodyfit_raster_interp_rows_device with the attribute rows of a face taken from a table of their own,
 *   A_a = attr[attr_faces[t][a]]   instead of   attr[faces[t][a]],
 * d_attr_faces int32 [n_faces][3] on the DEVICE and n_attr_rows the number of rows of d_attr (per frame); a non-zero
 * attr_frame_stride is >= n_channels n_attr_rows.  A uv atlas with seams is such a table: a vertex has several uv rows, and
 * n_attr_rows and n_verts are unrelated.  An entry of d_attr_faces outside [0, n_attr_rows) VOIDS the rows of that face (validated
 * on the device, as face ids are).  Everything else is bodyfit_raster_interp_rows_device's: the definition, the evaluation order,
 * the contract, the outputs and the error cases (plus: negative n_attr_rows, NULL d_attr_faces with n_channels > 0 and n_faces > 0);
 * with d_attr_faces = the topology's faces and n_attr_rows = n_verts the two entries return the same bits.  n_channels == 0 reads
 * no attributes and launches the un-indexed kernel.
 * With attr = the uv table, n_channels = 2 and d_grad_image = d_grad_uv of bodyfit_raster_texture_grad_device the rows are
 * dL/dverts of a textured image through the interpolation inside the faces.                                                       */
int bodyfit_raster_interp_rows_indexed_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames,
                                              double fx, double fy, double cx, double cy, const int32_t* d_face_image,
                                              const int32_t* d_pixel /* may be NULL */, const int32_t* d_offset /* may be NULL */,
                                              long long n_rows, const float* d_attr, long long attr_frame_stride, int n_channels,
                                              const int32_t* d_attr_faces, int n_attr_rows, const float* d_grad_image,
                                              const float* d_grad_z /* may be NULL */, int32_t* d_index,
                                              float* d_bary /* may be NULL */, float* d_dir /* may be NULL */,
                                              float* d_value /* may be NULL */, void* stream);
/* DISTANCE TRANSFORM with the nearest seed (a feature transform) of n_frames masks of the handle's size (k_edt.hip): what a
 * silhouette term needs of a person mask and of a rendered face-id image.  seed_kind 0: d_seed is u8 [n_frames][H][W] and a
 * pixel is a SEED iff its byte is != 0 (a bool image qualifies); seed_kind 1: d_seed is int32 [n_frames][H][W] and a pixel is
 * a seed iff its value is >= 0, so d_face of bodyfit_raster_render_device goes in as it is.  seed_frame_stride elements (bytes
 * or int32) between frames, >= H W.  invert != 0 swaps seeds and non-seeds.  The topology is not used: a handle with n_faces = 0
 * transforms masks without a mesh.  Outputs d_dist2 and, unless NULL, d_nearest: int32 [n_frames][H][W], dense, frame after frame.
 * DEFINITION, exact, in integers, for pixel (row i, column j) of frame f:
 *   dist2[f][i][j]   = min over the seeds (i', j') of frame f of (i - i')^2 + (j - j')^2,
 *   nearest[f][i][j] = i' W + j' of a seed that ATTAINS that minimum.
 * A seed pixel has dist2 0 and nearest itself.  A frame without a seed gets dist2 = INT32_MAX and nearest = -1 at every pixel.
 * Range: sizes are at most 16384 each way, so dist2 <= 2 x 16383^2 < 2^29, and every intermediate below is under 2^30: int32.
 * TIE RULE.  Among the seeds at the minimum the choice is a fixed function of the frame's mask: in a row the nearer seed column,
 * the LEFT one when two are equally near; down a column the row that entered the lower envelope first keeps every pixel at
 * which a later row only equals it.  So nearest is always the same one, but it is not "the lowest index": use it as A nearest
 * seed.
 * CONTRACT.  No tolerance: dist2 equals the definition at every pixel, and nearest is a seed of the same frame at exactly that
 * squared distance.  Every output element is written, whatever the outputs held.  No atomics of any kind, plain stores: the
 * results are bit-identical from run to run, and a frame's outputs depend on that frame only (identical whatever n_frames and
 * the stride).
 * Derivation.  Separable (Meijster, Roerdink, Hesselink 2000).  Row pass: c(i, j) = the seed column of row i nearest to j, from
 * leading / trailing-zero counts of the row's seed bits: exact by construction.  With g_i = (j - c(i, j))^2, the minimum over the
 * seeds of row i alone, dist2(x, j) = min_i F_i(x), F_i(x) = (x - i)^2 + g_i over the rows i that have a seed.  Column pass: the
 * lower envelope of these parabolas as a stack of (i, t_i): row i is a minimiser for x in [t_i, t_next).  For rows i < u,
 *   F_i(x) <= F_u(x)  <=>  2 x (u - i) <= u^2 - i^2 + g_u - g_i  <=>  x <= floor((u^2 - i^2 + g_u - g_i) / (2 (u - i)))
 * for INTEGER x, because u - i > 0 and an integer is <= a rational iff it is <= its floor.  Numerator and denominator are exact
 * int32 (below 2^30), and the quotient is the true floor (the truncated quotient, less one when the remainder is negative): no
 * rounding occurs anywhere, so the boundary t_u = 1 + that floor is the first integer row at which u is STRICTLY better than i,
 * not an approximation of the real intersection that could fall on the wrong side of an integer.  Row u pops the entries whose
 * first row it already beats strictly (F_i(t_i) > F_u(t_i)), which is the same exact comparison, and is dropped when t_u >= H.
 * Linear in the pixels: each row of a column is pushed and popped at most once.
 * Shape: one wave per (frame, row), the seeds as 64-bit ballots in LDS; one lane per (frame, column), neighbouring lanes on
 * neighbouring columns, the envelope stack in the workspace (8 bytes per pixel of a group of frames; the row pass's columns pass
 * through d_dist2 itself; a call of more than 2^29 pixels is worked group after group on the stream, so the workspace never
 * exceeds 4 GiB plus the slack of its growth).
 * Asynchronous on `stream`, NO host synchronisation (the workspace size follows from n_frames, H, W on the host); a call that has
 * to grow the workspace may synchronise, as the render does.  Calls on one handle share the workspace: order them.  n_frames ==
 * 0: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames, seed_kind not 0 or 1, and
 * with frames to write: NULL d_seed / d_dist2, a stride below H W.                                                             */
int bodyfit_raster_distance_device(bodyfit_raster* r, const void* d_seed, int seed_kind, long long seed_frame_stride,
                                   int n_frames, int invert, int32_t* d_dist2, int32_t* d_nearest /* may be NULL */,
                                   void* stream);
/* VERTEX ATTRIBUTES OVER A RENDER (k_rs_shade, k_raster_shade.hip): per-vertex attributes (colours) interpolated over a face-id image,
 * perspective-correct.  d_face int32 [n_frames][H][W] and d_bary f32 [n_frames][H][W][3]: a render of this handle's topology and
 * size, or hand-made images.  d_verts f32 [n_frames][n_verts][3], verts_frame_stride floats between frames (>= 3 n_verts); only
 * the z of the corners is read.  d_attr f32 rows of n_channels floats per vertex, n_channels in 1 .. 4; attr_frame_stride floats
 * between frames: 0 when the frames share one set of attributes, else >= n_channels n_verts.  background: 4 floats on the HOST, read
 * before the call returns (NULL: 0).  Outputs d_image f32 [n_frames][H][W][n_channels] and, unless NULL, d_weight f32
 * [n_frames][H][W][3], dense.  Every element of every frame is written, whatever the buffers held.
 * DEFINITION, exact from the f32 inputs.  At a pixel let t be its face id, ids = faces[t], Z_a the z of corner a, lambda_a its
 * three weights in d_bary, q_a = lambda_a / Z_a and S = sum_a q_a.  The pixel is VOID iff t is outside [0, n_faces), or some
 * lambda_a or Z_a is not finite, or some Z_a <= 0, or some lambda_a < 0, or S = 0.  A void pixel gets background[c] and weights 0.
 * Otherwise w_a = q_a / S and image[c] = sum_a w_a attr[ids[a]][c].  The w_a are the perspective-correct OBJECT-space weights of
 * the pixel's ray in the face: >= 0 and of sum 1 by construction; with the lambda of bodyfit_raster_render_device they are
 * lambda_a z / Z_a, z the rendered depth, up to that render's contract.  Attributes are plain IEEE: a NaN attribute gives NaN in
 * the pixels that use it.  d_weight is the (index, bary) of bodyfit_surface_rows_vjp_device for the gradient in the attributes.
 * CONTRACT, with u = 2^-24, k_s = 2 and per pixel and channel T_c = sum_a w_a |attr[ids[a]][c]|:
 *   |image^_c - image_c| <= k_s u T_c,        |w^_a - w_a| <= k_s u w_a
 * (for results in f32's normal range; one below 2^-126 is rounded to the subnormal grid, 2^-150 at most away).
 * Derivation (eps = 2^-53 = 2^-29 u; every operation f64, products and sums separately rounded, never fused).  The conversions
 * of lambda, Z and attr to f64 are exact.  Every q_a is >= 0, so nothing below cancels.  A quotient q_a: 1 eps.  S, two sums of
 * non-negative numbers: 3 eps.  w_a = q_a / S: 1 + 3 + 1 = 5 eps.  A product w_a attr_ac: 6 eps |w_a attr_ac|.  The channel's two
 * sums: 8 eps T_c.  The store rounds once: u |image^_c| <= u (1 + 8 eps) T_c.  Together (1 + 2^-25) u T_c, stated as k_s = 2; a
 * weight is 5 eps and the store's u: the same k_s.
 * One thread per pixel, neighbouring lanes on neighbouring columns; each gathers the face's three ids, three z and 3 n_channels
 * attributes (neighbouring pixels mostly share a face); plain stores, no atomics, no workspace: bit-identical from run to run, and
 * a frame's image depends on that frame only (bit-identical whatever n_frames; with or without d_weight).  Asynchronous on
 * `stream`, no host synchronisation.  n_frames == 0: a successful no-op; n_faces == 0: every pixel background.
 * BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames, n_channels outside 1 .. 4, and with frames to write:
 * NULL d_face / d_bary / d_image, NULL d_verts or d_attr (n_faces > 0), a vertex stride below 3 n_verts, a non-zero attribute
 * stride below n_channels n_verts, 2^39 pixels or more.                                                                        */
int bodyfit_raster_shade_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                long long verts_frame_stride, const float* d_attr, long long attr_frame_stride, int n_channels,
                                int n_frames, const float* background /* host [4]; may be NULL */, float* d_image,
                                float* d_weight /* may be NULL */, void* stream);
/* IMAGE SAMPLES AT PROJECTED POINTS (k_rs_sample, k_raster_shade.hip): a batch of images read bilinearly where the points of a cloud
 * project, with the image gradient there.  The topology is not used: a handle with n_faces = 0 samples images (of its size), as
 * it transforms masks.  d_points f32 [n_frames][n_points][3], points_frame_stride floats between frames (>= 3 n_points:
 * bodyfit_device_views.cloud is used in place); intrinsics in f64 (fx, fy > 0), z_near > 0.  d_image: image_kind 0 = u8, 1 = f32,
 * [n_frames][H][W][n_channels] interleaved, n_channels in 1 .. 4, image_frame_stride ELEMENTS between frames (>= H W n_channels);
 * a u8 texel is its raw value 0 .. 255, not scaled.  d_gate u8 [n_frames][n_points] or NULL.  Outputs d_value f32
 * [n_frames][n_points][n_channels], d_valid u8 [n_frames][n_points] and, unless NULL, d_grad f32 [n_frames][n_points]
 * [n_channels][2] = (d/du, d/dv).  Every element is written; an invalid point gets 0 everywhere.
 * DEFINITION.  (u, v) = (fx X / Z + cx, fy Y / Z + cy); pixel centres at integers, the render's convention.  A point is LIVE iff
 * X, Y, Z are finite, Z >= z_near, its gate byte is non-zero (or d_gate is NULL), 0 <= u <= W - 1 and 0 <= v <= H - 1.  For a live
 * point j0 = min(floor(u), max(W - 2, 0)), j1 = min(j0 + 1, W - 1), a = u - j0, and i0, i1, b alike in v, H;
 *   value_c = (1 - a)(1 - b) I[i0][j0] + a (1 - b) I[i0][j1] + (1 - a) b I[i1][j0] + a b I[i1][j1],
 *   d/du    = (1 - b)(I[i0][j1] - I[i0][j0]) + b (I[i1][j1] - I[i1][j0]),
 *   d/dv    = (1 - a)(I[i1][j0] - I[i0][j0]) + a (I[i1][j1] - I[i0][j1]):
 * the exact derivative of the bilinear patch of the cell (i0, j0) (at u = W - 1 the last cell's, from the left; W = 1: 0).
 * CONTRACT, with u = 2^-24, P = max(W, H) + max(|cx|, |cy|), delta = 2^-50 P and M the largest |texel| among the texels of the
 * exact cell and of the returned cell:
 *   (a) a point that is live and at least delta inside the border is returned live; a point returned live lies within delta of
 *       the closed rectangle [0, W - 1] x [0, H - 1]; the tests on Z, on the gate and on finiteness are exact;
 *   (b) |value^ - B(u, v)| <= u |B| + 2^-46 P M, B the continuous bilinear surface through the texels;
 *   (c) there is a cell K whose closed support is within delta of the exact (u, v) such that each returned derivative is within
 *       u |g_K| + 2^-46 P M of the derivative g_K of K's patch at (u, v).
 * Derivation (eps = 2^-53; every operation f64 and unfused).  u^: the quotient, the product and the sum round once each, 3 eps P
 * = 2^-51.4 P, as in the render's derivation: inside delta.  The comparisons and floor act on u^, which gives (a), and the
 * returned cell K holds (u^, v^) in its closed support, within delta of (u, v).  a = u^ - j0 is exact (Sterbenz, or j0 = 0 and a =
 * u^).  B is continuous and piecewise bilinear, of slope at most 2 M per pixel in each coordinate, and equals K's patch at (u^,
 * v^): moving from (u, v) to (u^, v^), at most delta each way, changes it by at most 4 M delta = 2^-48 P M.  The patch evaluated in
 * f64: 1 - a, four products of two weights, four products with texels, three sums: below 8 eps M.  Together below 2^-47 P M,
 * stated as 2^-46 P M; the store rounds once: u |B|.  A derivative of K's patch is linear in the other coordinate with slope at
 * most 4 M: 4 M delta = 2^-48 P M for the move, differences of texels are exact for u8 and 1 eps for f32, two products and a sum:
 * below 8 eps M; the store's u |g_K|.
 * One thread per (frame, point); the 4 n_channels texels are gathered before anything is combined.  Plain stores, no atomics, no
 * workspace: bit-identical from run to run, and a frame's outputs depend on that frame only.  Asynchronous on `stream`, no host
 * synchronisation.  n_frames == 0 or n_points == 0: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle,
 * negative n_frames or n_points, n_channels outside 1 .. 4, image_kind outside {0, 1}, z_near <= 0 or NaN, fx or fy <= 0 or a
 * non-finite intrinsic, and with points to write: NULL d_points / d_image / d_value / d_valid, a point stride below 3 n_points,
 * an image stride below H W n_channels, 2^39 points or more.                                                                 */
int bodyfit_raster_sample_device(bodyfit_raster* r, const float* d_points, long long points_frame_stride, long long n_points,
                                 int n_frames, double fx, double fy, double cx, double cy, float z_near, const void* d_image,
                                 int image_kind, int n_channels, long long image_frame_stride,
                                 const uint8_t* d_gate /* may be NULL */, float* d_value, uint8_t* d_valid,
                                 float* d_grad /* may be NULL */, void* stream);
/* UV TEXTURES OVER A RENDER (k_tx_forward, k_texture.hip): the texture lookup of Laine et al. (2020) without its mipmaps.
 * ATLAS.  d_uv f32 [n_uv][2] and d_uv_faces int32 [n_faces][3], both on the device: the rows of d_uv per face CORNER.  An atlas has
 * seams, so a vertex has several uv rows: n_uv and n_verts are unrelated.  TEXTURE.  d_tex: tex_kind 0 = u8 (a texel is its raw
 * value 0 .. 255, as in bodyfit_raster_sample_device), 1 = f32; [Ht][Wt][n_channels] interleaved, n_channels in 1 .. 4, Ht and Wt in
 * 1 .. 16384; tex_frame_stride ELEMENTS between the frames' textures: 0 when the frames share one, else >= Ht Wt n_channels.
 * TEXEL POSITIONS.  Texel (i, j) has its centre at (u, v) = ((j + 1/2) / Wt, (i + 1/2) / Ht); row 0 is at the top, nothing is flipped.
 * x = u Wt - 1/2, y = v Ht - 1/2.  Addressing is CLAMP-TO-EDGE: x is clamped to [0, Wt - 1] and y to [0, Ht - 1], in f64 and BEFORE
 * anything is converted to an integer, so a huge or negative uv never becomes an index; then the cell, a and b are the sampler's:
 * j0 = min(floor(x), max(Wt - 2, 0)), j1 = min(j0 + 1, Wt - 1), a = x - j0, and i0, i1, b alike in y, Ht (one device helper,
 * bilinear_inl.h, serves both kernels).
 * d_face, d_bary, d_verts (only the corners' z is read), verts_frame_stride, background and the VOID rule are exactly
 * bodyfit_raster_shade_device's; in addition a pixel is void when an entry of d_uv_faces of its face is outside [0, n_uv) (validated
 * on the device) or when its u or v is not finite.  Outputs, dense, every element of every frame written whatever the buffers held:
 * d_image f32 [n_frames][H][W][n_channels]; unless NULL d_weight f32 [n_frames][H][W][3] and d_uv_out f32 [n_frames][H][W][2].
 * DEFINITION.  w_a are the shade's weights, formed by the same operations in the same order (d_weight equals the shade's bit for
 * bit wherever both shade the pixel); with uv_a = uv[uv_faces[t][a]], per component (u, v) = (w_0 uv_0 + w_1 uv_1) + w_2 uv_2;
 *   image_c = (1 - a)(1 - b) T[i0][j0] + a (1 - b) T[i0][j1] + (1 - a) b T[i1][j0] + a b T[i1][j1]
 * at the clamped (x, y).  A void pixel gets background[c], weights 0 and uv 0.  Texels are plain IEEE.
 * CONTRACT, with u = 2^-24, U = max(1, max_a |u_a|, max_a |v_a|) over the face's three uv rows, P_x = max(Wt, Ht), delta = 2^-49 P_x U,
 * kappa = k_t 2^-50 P_x U with k_t = 16, B the continuous clamp-to-edge bilinear surface through the texels and M the largest
 * |texel| among the texels of the exact cell and of the returned cell, at every pixel that is not void:
 *   |image^_c - B_c(x, y)| <= u |B_c| + kappa M,     |uv^ - uv| <= k_s u sum_a w_a |uv_a| per component (k_s = 2, the shade's),
 * the returned (x^, y^) is within delta of the exact clamped (x, y), and d_weight is the shade's.  A pixel whose exact u or v
 * overflows nothing here: |uv_a| <= 2^128 and Wt <= 2^14 stay far inside f64.
 * Derivation (eps = 2^-53; every operation f64 and unfused).  w_a: 5 eps (the shade's derivation).  A product w_a u_a (u_a exact in
 * f64): 6 eps; the two sums: |du| <= 8 eps sum_a w_a |u_a| <= 8 eps U (1 + 5 eps) (the exact w_a sum to 1).  x^ = u^ Wt - 1/2: the
 * product and the difference round once each, on magnitudes <= Wt U + 1/2: |dx| <= (8 + 1 + 1.5) eps Wt U <= 11 eps P_x U < delta
 * = 16 eps P_x U.  The clamp is monotone and does not expand distances: the clamped x^ is within delta of the clamped x; a = x^ - j0
 * is exact (Sterbenz, or j0 = 0).  B is continuous and piecewise bilinear with slope at most 2 M per texel in each coordinate (0
 * outside the texel centres' rectangle) and equals the returned cell's patch at (x^, y^): moving by delta each way changes it by at
 * most 4 M delta = 8 x 2^-50 P_x U M.  The patch in f64 (1 - a, 1 - b, four weight products, four texel products, three sums):
 * below 8 eps M = 2^-50 M.  Together 9 x 2^-50 P_x U M, stated as k_t = 16; the store rounds once: u |B|.
 * One thread per pixel, neighbouring lanes on neighbouring columns; the gathers are the shade's plus 24 bytes of uv and the 4
 * n_channels texels.  Plain stores, no atomics, no workspace: bit-identical from run to run, and a frame's outputs depend on that
 * frame only.  Asynchronous on `stream`, no host synchronisation.  n_frames == 0: a successful no-op; n_faces == 0: every pixel
 * background.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames or n_uv, n_channels outside 1 .. 4, tex_kind
 * outside {0, 1}, Ht or Wt outside 1 .. 16384, a non-zero texture stride below Ht Wt n_channels, and with frames to write: NULL
 * d_face / d_bary / d_image, NULL d_verts / d_uv_faces / d_tex (n_faces > 0), NULL d_uv (n_faces > 0 and n_uv > 0), a vertex stride
 * below 3 n_verts, 2^39 pixels or more.
 * NOT BUILT HERE: wrap and mirror addressing.  THIS entry has no minification filter: a body that is smaller on the screen than its
 * atlas ALIASES (a pixel reads one 2 x 2 cell, whatever area of the atlas it covers), and the texels no pixel's cell touches receive
 * no gradient.  bodyfit_raster_texture_mip_device (MIPMAPS OF THE TEXTURE LOOKUP, below) is the lookup with mipmaps.            */
int bodyfit_raster_texture_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                  long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                  const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                  long long tex_frame_stride, int n_frames, const float* background /* host [4]; may be NULL */,
                                  float* d_image, float* d_weight /* may be NULL */, float* d_uv_out /* may be NULL */,
                                  void* stream);
/* THE LOOKUP'S GRADIENTS (k_tx_gmax, k_tx_grad, k_tx_fold, k_texture.hip) for an upstream G = d_grad_image f32 [n_frames][H][W]
 * [n_channels] = dL/dimage; the other inputs are bodyfit_raster_texture_device's, and the pixel (void rule, weights, uv, clamp,
 * cell) is evaluated again by the same device function.  Two results, each skipped when its pointer is NULL:
 * (a) d_grad_uv f32 [n_frames][H][W][2] = (sum_c G_c dimage_c/du, sum_c G_c dimage_c/dv) in uv units: the exact derivative of the
 *     cell's patch (bodyfit_raster_sample_device's d/du, d/dv) times Wt and Ht; a component is 0 where its clamp is ACTIVE (the
 *     unclamped x outside [0, Wt - 1], y alike) and both are 0 where the pixel is void.  Order: sum_c as ((G_0 d_0 + G_1 d_1) + G_2 d_2) +
 *     G_3 d_3, then the product with Wt.  Plain stores, every element written.  Needs d_tex.
 * (b) d_grad_tex f32 in the texture's layout, [Ht][Wt][n_channels] when the frames share the texture (tex_frame_stride == 0: summed
 *     over ALL frames) and dense [n_frames][Ht][Wt][n_channels] otherwise, for u8 and f32 textures alike: the exact adjoint of the
 *     lookup in the texels, g*[i][j][c] = sum over the pixels whose cell holds texel (i, j) of G_c omega_k, omega_k the texel's
 *     bilinear weight (1 - a)(1 - b), a (1 - b), (1 - a) b or a b at the pixel's returned (x^, y^); where the clamp or a 1-wide texture
 *     makes two texels of the cell coincide both contributions go to it.  Every element is written.  d_tex is not read for (b).
 * HOW (b) IS SUMMED: EXACTLY, IN INTEGERS, without float atomics (a many-to-few scatter has no usable order; k_winding.hip's rule).
 *   1. One pass finds Gmax = max |G| over the WHOLE of d_grad_image (void pixels included) as the u32 bit pattern of |G|: a wave
 *      reduction and one integer atomicMax per workgroup.  For non-negative floats the patterns order as the values, and every NaN or
 *      infinity has a pattern >= 0x7f800000.  It stays on the device: no host synchronisation.
 *   2. E = (pattern >> 23) - 126 is the smallest exponent with Gmax < 2^E that the pattern's exponent field gives.  With N = n_frames H
 *      W (known on the host) and B its bit length (N < 2^B),  s = 60 - B - E  ( = 62 - (B + 2) - E ).  A texel receives at most 4 N
 *      contributions, each |G_c omega_k| <= Gmax < 2^E since 0 <= omega_k <= 1, so every partial sum of the integers below is under
 *      4 N 2^(E + s) < 2^(B + 2) 2^(60 - B) = 2^62: no overflow, whatever the order.  With s + 1 the same bound is >= 2^62.
 *   3. A contribution is t = fl(G_c omega_k) in f64 (omega_k from bilinear_inl.h's four products; the product with G_c rounds once),
 *      scaled by 2^s (exact: |s| <= 186, a power of two) and converted with round-to-nearest-even to an int64 q; q != 0 is added with
 *      a no-return 64-bit INTEGER atomic into d_workspace, int64 [Ht][Wt][n_channels] (x n_frames for per-frame textures), which the
 *      entry zeroes on the stream.  Contributions that are exactly 0 are skipped.
 *   4. A fold kernel writes (float)((double)sum 2^-s).
 * Integer addition is associative and commutative, so d_grad_tex is bit-identical from run to run, for any launch geometry, and
 * for ANY PERMUTATION OF THE FRAMES (of a shared texture; per-frame textures permute with them).
 * DEGENERATE Gmax.  Gmax = 0: d_grad_tex and d_grad_uv are all 0.  A NaN or an infinity ANYWHERE in d_grad_image: d_grad_tex is
 * all NaN and d_grad_uv all 0 (nothing is accumulated: the conversion of a non-finite value to an integer is never reached).
 * CONTRACT, with u = 2^-24, eps = 2^-53, kappa and M of the lookup, k_g = 6, and per texel element m = the number of its non-zero
 * contributions and A = sum |G_c omega_k| over them:
 *   (a) there is a cell K whose closed support is within delta of the exact clamped (x, y), the returned one, such that
 *       |g^_u - g_u| <= u |g_u| + kappa Wt M sum_c |G_c|   with g_u = Wt sum_c G_c (d/du of K's patch at (x, y)); v alike with Ht; the
 *       decision "the clamp is active" is exact for an unclamped x at least delta from 0 and Wt - 1 and either way inside;
 *   (b) |g^ - g*| <= u |g*| + m 2^-(s + 1) + k_g eps A.
 * Derivation.  (a): a derivative of K's patch is linear in the other coordinate with slope at most 4 M: 4 M delta for the move;
 * differences of texels 1 eps, two products and a sum: below 8 eps M; the sum over the channels (n_channels + 1) eps more, the
 * product with Wt one more: (4 delta + 14 eps) M Wt sum |G_c| <= 10 x 2^-50 P_x U Wt M sum |G_c|, inside kappa; the store's u.  (b):
 * 1 - a and 1 - b round once, the weight's product once: omega^ within 3 eps of omega; the product with G_c: 4 eps |G_c omega_k|;
 * the scaling is exact and the conversion moves each contribution by at most 1/2 unit of 2^-s: m 2^-(s + 1); the integer sum is
 * exact; (double)sum rounds once when |sum| >= 2^53 (1 eps of at most A (1 + ...)), the product with 2^-s is exact, the store rounds
 * once: u.  Together 5 eps A, stated as k_g = 6.  Against the exact positions (x, y) instead of the returned ones each omega moves by
 * at most 2 delta: add 2 delta sum |G_c| over the texel's pixels.  In f32 terms: with N = 2^21 pixels of |G| <= 1, s = 38 and a
 * texel hit by 10^4 pixels carries an absolute error below 2^-25 from the conversion: under the store's rounding of anything >= 1.
 * Shape: one thread per pixel for the pass that adds.  Neighbouring pixels share cells under magnification, so the lanes of a wave
 * first add their integers up over each RUN of consecutive lanes with the same cell (a segmented suffix sum by shuffles, exact:
 * integers) and the run's first lane issues its 4 n_channels atomics; a wave without a covered pixel skips all of it.  The sums
 * are the same bits as with one atomic per contribution (measured: DESIGN.md section 5, "Textures").
 * Asynchronous on `stream`, NO host synchronisation.  Calls on one handle share one u32 of device state (Gmax): order them, as
 * calls that share the render's workspace.  n_frames == 0, or both outputs NULL: a successful no-op.  BODYFIT_ERR_INVALID (nothing
 * is launched): every case of bodyfit_raster_texture_device but those of d_image and d_tex, and with frames to write: NULL
 * d_grad_image, d_grad_tex without d_workspace, d_grad_uv without d_tex (n_faces > 0), 2^39 texel elements or more.
 * NOT BUILT: the term's normal equations, the C++ mirror header's entry.                                                      */
int bodyfit_raster_texture_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                       long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                       const void* d_tex /* may be NULL without d_grad_uv */, int tex_kind, int n_channels,
                                       int tex_height, int tex_width, long long tex_frame_stride, int n_frames,
                                       const float* d_grad_image, float* d_grad_uv /* may be NULL */,
                                       float* d_grad_tex /* may be NULL */, long long* d_workspace /* may be NULL without d_grad_tex */,
                                       void* stream);
/* MIPMAPS OF THE TEXTURE LOOKUP (k_txm_build, k_txm_forward, k_txm_grad, k_txm_fold, k_texture.hip): the minification filter of
 * Laine et al. (2020): a pyramid of the texture, a level of detail per pixel from the face's footprint, and a trilinear lookup.
 * The entries above are unchanged; these stand next to them.
 * THE PYRAMID.  Level 0 is the texture.  Level l + 1 exists iff l < max_level (max_level < 0: as many as exist), (H_l, W_l) != (1, 1)
 * and each of H_l, W_l is EVEN OR 1; a dimension > 1 is halved, a dimension of 1 stays 1.  There are no odd halvings: a texel of level
 * l + 1 is exactly the union of its children in uv, so the texel-centre convention above holds on every level with (W_l, H_l) for
 * (Wt, Ht).  7 x 5 has one level, 12 x 20 three (12 x 20, 6 x 10, 3 x 5), 1 x 8 four, 64 x 64 seven, 16384 x 16384 fifteen =
 * BODYFIT_TX_MAX_LEVELS.  bodyfit_texture_mip_layout (host only, no GPU): *n_levels, heights[l] = H_l, widths[l] = W_l and offsets[l],
 * the TEXEL offset of level l in a packed buffer that holds levels 1 .. n_levels - 1 (offsets[0] = 0 is not used), for l < n_levels
 * (each array BODYFIT_TX_MAX_LEVELS long, or NULL), and *total, that buffer's texels.  BODYFIT_ERR_INVALID: a size outside 1 ..
 * 16384, NULL n_levels.
 * bodyfit_raster_texture_mip_build_device writes d_mip f32: per texture the levels 1 .. n_levels - 1, level l at offsets[l] n_channels,
 * [H_l][W_l][n_channels] interleaved; textures mip_frame_stride ELEMENTS apart (>= total n_channels; not used with n_textures = 1).
 * Level l + 1 is built from the STORED level l (d_tex in its own type for l = 0, the f32 level otherwise):
 *   ((t00 + t01) + (t10 + t11)) * 0.25   over the children (2i, 2j), (2i, 2j + 1), (2i + 1, 2j), (2i + 1, 2j + 1), in f64, rounded once to
 * f32;  (t0 + t1) * 0.5 over the two children where one dimension is 1.  One thread per output element, plain stores, one launch per
 * level: bit-identical from run to run.  Asynchronous on `stream`, no host synchronisation.  n_textures == 0 or one level: a no-op.
 * BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_textures, n_channels, tex_kind or a size out of range, with
 * n_textures > 1 a texture stride below Ht Wt n_channels or (more than one level) a pyramid stride below total n_channels, and with
 * levels to write NULL d_tex or d_mip, 2^39 elements or more.
 * THE LOOKUP WITH A LEVEL OF DETAIL, bodyfit_raster_texture_mip_device: the arguments of bodyfit_raster_texture_device, the render's
 * fx, fy, cx, cy, the pyramid (d_mip, mip_frame_stride; with tex_frame_stride == 0 ONE pyramid serves every frame and the stride is
 * not used), max_level (the one the pyramid was built with), lod_bias, and unless NULL d_lod f32 [n_frames][H][W]: the L that was
 * used, 0 on void pixels.  The void rule, the weights w_a, uv and the clamp are the plain lookup's (the same device function):
 * d_weight and d_uv_out are its bits.  All of d_verts' coordinates are read here.
 * FOOTPRINT, analytically from the face (no differences of neighbouring pixels).  p_a = (fx X_a / Z_a + cx, fy Y_a / Z_a + cy), A =
 * (p1 - p0) x (p2 - p0) the render's doubled area, grad lambda_a = (p_b,y - p_c,y, p_c,x - p_b,x) / A (b, c the corners after a); with
 * q_a = lambda_a / Z_a of the stored barycentrics and S = sum q_a:  d(uv)/ds = sum_a (grad lambda_a / Z_a)(uv_a - uv) / S, a 2 x 2
 * matrix; J = diag(Wt, Ht) d(uv)/ds in level-0 texels per pixel; rho^2 the largest eigenvalue of J J^T (rotation-invariant),
 *   rho^2 = (a + b) / 2 + sqrt(((a - b) / 2)^2 + c^2),   a, b the squared norms of J's columns, c their dot product;
 *   L = clamp(log2(rho^2) / 2 + lod_bias, 0, n_levels - 1).
 * L = 0 where rho^2 is NaN or +inf, where A = 0 or is not finite, or where an X or Y of the face is not finite (the plain rule only
 * looks at Z; hand-made face images reach such faces); rho^2 = 0 gives -inf and clamps to 0; lod_bias may be -inf or +inf.
 * Order (f64, unfused): p_a as the render's; A as the render's; h_a = ((p_b,y - p_c,y) / A) / Z_a and ((p_c,x - p_b,x) / A) / Z_a;
 * d_a = uv_a - uv^; ((h_0 d_0 + h_1 d_1) + h_2 d_2) / S; the product with Wt or Ht; a = J00 J00 + J10 J10, b, c alike; hs = 0.5 (a +
 * b), hd = 0.5 (a - b); rho^2 = hs + sqrt(hd hd + c c); 0.5 log2(rho^2) + lod_bias; the clamp; THE ROUNDING TO f32: the f32 in d_lod
 * IS the L that the filter and the gradients use, so everything below that is stated "at the returned L^" can be checked from d_lod.
 * FILTER.  l0 = floor(L), f = L - l0 (exact).  P_l is the clamp-to-edge bilinear patch of level l at the pixel's uv, each level with
 * its OWN clamp and cell (x_l = u W_l - 1/2, ...; the same helpers).  image_c = (1 - f) P_l0 + f P_(l0+1): 1 - f, two products and a
 * sum in f64, rounded once.  WHERE f = 0 ONLY LEVEL l0 IS READ and image_c = P_l0 with no blend arithmetic: with a lod_bias that
 * forces L = 0 everywhere (-inf, -1000), or with a one-level texture, d_image is BIT-IDENTICAL to bodyfit_raster_texture_device's,
 * and a NaN in a level that is not used cannot leak in.
 * CONTRACT.  With the plain lookup's u, U, P_x, kappa (of level 0: the largest of the levels'), the render's P_t, Q_t, R_t of the face,
 * Lambda = the sum of the pixel's three stored barycentrics, eps = 2^-53 and
 *   D = 12 U R_t Q_t / (P_t Lambda)              (no entry of d(uv)/ds exceeds it),
 *   E_J = k_J eps P_x D (1 + 4 Q_t), k_J = 64     (the computed rho^ is within E_J of rho),
 *   d_log = k_L eps (1 + |log2(rho^2) / 2| + |lod_bias|), k_L = 24,
 * the returned L^ is the f32 rounding (u L) of a value in [clamp(log2(max(rho - E_J, 0)) + lod_bias - d_log), clamp(log2(rho + E_J) +
 * lod_bias + d_log)]; delta_L is the larger distance of that interval's ends from the exact L, plus u L.  It holds for 80 eps Q_t <= 1/2;
 * a face beyond that (a sliver whose area is lost in P_t^2) has delta_L = n_levels - 1: nothing is said about its level.  With
 * I(L) = (1 - f) B_l0 + f B_(l0+1) over the STORED pyramid, B_l the continuous surface of level l, and M the largest |texel| among the
 * exact and the returned cells of every level from floor(L - delta_L) to ceil(L + delta_L):
 *   |image^_c - I_c(L)| <= u |I_c| + kappa M + 2 M delta_L,     and at the returned level   |image^_c - I_c(L^)| <= u |I_c| + kappa M.
 * Derivation.  A coordinate of p_a: 3 eps P_t; a difference of two: 8 eps P_t against |.| <= 2 P_t; A: 80 eps P_t^2 (the render's
 * derivation), relative 80 eps Q_t.  (p_b,y - p_c,y) / A: at most g = 2 P_t / |A| = 2 Q_t / P_t, off by g eps (5 + 80 Q_t) to first
 * order; / Z_a: one more, at most g / Z_min.  d_a: uv^ is within 8 eps U of uv (the plain derivation), the difference rounds: 10 eps U
 * against |d_a| <= 2 U.  A product h_a d_a <= T = 2 U g / Z_min, off by T eps (13 + 80 Q_t); the sum of three: 3 T eps (15 + 80 Q_t).
 * S >= Lambda / Z_max, computed within 3 eps; the quotient: entries <= 3 T Z_max / Lambda = D, off by D eps (19 + 80 Q_t); the product
 * with Wt or Ht: P_x D eps (20 + 80 Q_t).  The largest singular value moves by at most the Frobenius norm of the change of J, 2 entries
 * a side: |rho^ - rho| <= 2 P_x D eps (20 + 80 Q_t) = 40 eps P_x D (1 + 4 Q_t), stated as k_J = 64 for the terms of second order.
 * a, b, c, hs, hd and the sum under the root carry at most 12 eps (a + b) <= 24 eps rho^2 into rho^2; sqrt is correctly rounded and
 * log2 is within 1 ulp on the device (the ROCm device library's documented accuracy for f64): 18 eps + 2 eps |log2(rho^2) / 2|, the sum
 * with lod_bias one more: inside d_log.  The filter is CONTINUOUS in L (at f -> 1 it is P_(l0+1), which is the next interval's f = 0)
 * with slope P_(l0+1) - P_l0, at most 2 M: a wrong floor next to an integer L costs 2 M delta_L like any other error in L.  Each patch
 * is within kappa_l M of its surface before the store (the plain derivation, 9 of the 16 units), the blend adds 3 eps M.
 * THE GRADIENTS, bodyfit_raster_texture_mip_grad_device (k_tx_gmax, k_txm_grad, k_txm_fold), at the FIXED face image, pixel rays and
 * LEVEL OF DETAIL: L and f are constants; the gradient through rho is NOT built.
 * (a) d_grad_uv = (1 - f) [level l0's patch derivative times (W_l0, H_l0)] + f [level l0 + 1's, likewise], each level with its own
 *     clamp-active rule, the plain order inside a level, then 1 - f, two products and a sum; where f = 0 the single-level form, which
 *     for l0 = 0 is the plain entry's bit for bit.  Contract at the returned L^: the plain (a) per level, blended with (1 - f, f), plus
 *     the store's u |g|; against the exact L add 4 M P_x delta_L sum_c |G_c| (the blend is continuous in L, a level's g is at most
 *     2 M P_x sum_c |G_c|).
 * (b) d_grad_tex in the LEVEL-0 texture's layout (shared: summed over all frames): the exact adjoint of "build the pyramid by
 *     UNROUNDED averaging, then filter".  A pixel contributes fl(G_c fl((1 - f) omega_k)) to its 4 texels of level l0 and, where f !=
 *     0, fl(G_c fl(f omega'_k)) to its 4 texels of level l0 + 1 (f = 0: fl(G_c omega_k), the plain contribution); each is scaled by 2^s,
 *     rounded to int64 and added with a no-return 64-bit INTEGER atomic into d_workspace, int64 with the pyramid's packed layout and
 *     LEVEL 0 FIRST: (Ht Wt + total) n_channels elements per texture, level l >= 1 at (Ht Wt + offsets[l]) n_channels; the entry zeroes
 *     it.  s = 60 - B - E holds as it is: PER LEVEL a texel still receives at most 4 N contributions (a pixel gives a level at most 4),
 *     each |G_c share omega_k| <= Gmax < 2^E since 0 <= (1 - f), f, omega_k <= 1: every partial sum stays under 2^62.  Gmax = 0, NaN and
 *     infinity are handled as in the plain entry (k_tx_gmax is the same kernel).
 *     FOLD, one thread per level-0 texel element (i, j, c): in f64 and in the fixed order l = 0, 1, ..., n_levels - 1,
 *       acc = (double)S_0[i][j][c] 2^-s;   acc = acc + ((double)S_l[i_l][j_l][c] 2^-s) a_l,
 *     (i_l, j_l) the texel's ancestor on level l (a halved dimension shifts right by one per level) and a_l the exact power of two that
 *     is the product of the build's 1/4 and 1/2 factors; the float of acc is stored.  The scatter is bit-identical by integer
 *     associativity, the fold is a fixed-order gather: d_grad_tex is bit-identical from run to run and for any permutation of the
 *     frames.  With one level, or L = 0 everywhere, it is the plain entry's bit for bit.
 *     Contract, with m_l and A_l the plain (b)'s m and A of the texel's ancestor on level l, against g* = sum_l a_l S*_l (S*_l the exact
 *     sums at the returned cells, weights and L^), k_m = 24:
 *       |g^ - g*| <= u |g*| + sum_l a_l m_l 2^-(s + 1) + k_m eps sum_l a_l A_l.
 *     Derivation: omega^ within 3 eps, 1 - f one, the share's product one, the product with G_c one: 6 eps A_l; (double)S_l one; the
 *     n_levels - 1 <= 14 sums of the fold one each on partial sums <= sum_l a_l A_l: together below 22 eps, stated as 24.
 * RUN COMBINING (BODYFIT_TXM_COMBINE) is the plain entry's with the key (level, cell) of both of a lane's levels; the bits are the
 * same either way.  Both forms were measured on a magnified and on a minified render ("Mipmaps"): combining is
 * the faster on both and is the default (1).  The per-lane integers and addresses are indexed with compile-time constants only (the
 * one or two levels are unrolled): the kernels use no scratch memory.
 * The vertex gradient is the plain path's: d_grad_uv through bodyfit_raster_interp_rows_indexed_device and the rows VJP.
 * Asynchronous on `stream`, no host synchronisation; the Gmax word is shared as in the plain entry.  BODYFIT_ERR_INVALID (nothing is
 * launched): every case of the plain entries, and fx or fy <= 0 or a non-finite intrinsic, a NaN lod_bias, NULL d_mip with more than
 * one level (the gradient entry: only with d_grad_uv), with per-frame textures a pyramid stride below total n_channels, 2^39
 * workspace elements or more.
 * NOT BUILT: the gradient through the level of detail, anisotropic filtering, wrap and mirror addressing, caller-supplied pyramids
 * (the lookup reads what the build entry's layout says), a mip-aware bake (torch_layer.bake_texture stays level 0), the term's
 * normal equations, the C++ mirror header's entries.                                                                            */
#define BODYFIT_TX_MAX_LEVELS 15
int bodyfit_texture_mip_layout(int tex_height, int tex_width, int max_level, int* n_levels, int* heights /* may be NULL */,
                               int* widths /* may be NULL */, long long* offsets /* may be NULL */, long long* total /* may be NULL */);
int bodyfit_raster_texture_mip_build_device(bodyfit_raster* r, const void* d_tex, int tex_kind, int n_channels, int tex_height,
                                            int tex_width, long long tex_frame_stride, int n_textures, int max_level, float* d_mip,
                                            long long mip_frame_stride, void* stream);
int bodyfit_raster_texture_mip_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                      long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                      const void* d_tex, int tex_kind, int n_channels, int tex_height, int tex_width,
                                      long long tex_frame_stride, int n_frames, double fx, double fy, double cx, double cy,
                                      const float* d_mip /* may be NULL with one level */, long long mip_frame_stride, int max_level,
                                      float lod_bias, const float* background /* host [4]; may be NULL */, float* d_image,
                                      float* d_weight /* may be NULL */, float* d_uv_out /* may be NULL */,
                                      float* d_lod /* may be NULL */, void* stream);
int bodyfit_raster_texture_mip_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                           long long verts_frame_stride, const float* d_uv, int n_uv, const int32_t* d_uv_faces,
                                           const void* d_tex /* may be NULL without d_grad_uv */, int tex_kind, int n_channels,
                                           int tex_height, int tex_width, long long tex_frame_stride, int n_frames, double fx,
                                           double fy, double cx, double cy, const float* d_mip /* may be NULL without d_grad_uv */,
                                           long long mip_frame_stride, int max_level, float lod_bias, const float* d_grad_image,
                                           float* d_grad_uv /* may be NULL */, float* d_grad_tex /* may be NULL */,
                                           long long* d_workspace /* may be NULL without d_grad_tex */, void* stream);
/* LIGHTING OF A RENDER (k_lt_forward, k_light.hip): second-order spherical-harmonic shading, image = albedo x shading(normal).
 * d_face, d_bary, d_verts (only the corners' z is read), verts_frame_stride and the VOID rule are exactly
 * bodyfit_raster_shade_device's.  d_normals f32 [n_frames][n_verts][3], normals_frame_stride floats between frames (>= 3 n_verts):
 * per-vertex normals, bodyfit_surface_vertex_normals_device's or any others; they need not be unit.  d_albedo f32 [n_frames][H][W]
 * [n_channels], n_channels in 1 .. 4: an image that bodyfit_raster_shade_device or a texture lookup made, background included.
 * d_light f32 [9][n_channels], light_frame_stride floats between the frames' lights: 0 when the frames share one, else >= 9
 * n_channels.  Outputs, dense, every element of every frame written whatever the buffers held: d_image f32 [n_frames][H][W]
 * [n_channels]; unless NULL d_normal f32 [n_frames][H][W][3] and d_shading f32 [n_frames][H][W][n_channels].
 * DEFINITION, exact from the f32 inputs.  w_a are the shade's weights, formed by the same operations in the same order (bit-equal
 * to its d_weight before the store).  With n_a the normal of corner a:  m = (w_0 n_0 + w_1 n_1) + w_2 n_2 per component,
 * l = |m| = sqrt((m_x^2 + m_y^2) + m_z^2), n = m / l = (x, y, z),
 *   b(n) = (1, x, y, z, x y, x z, y z, x^2 - y^2, 3 z^2 - 1),   s_c = sum_k light[k][c] b_k (ascending k),   image_c = albedo_c s_c.
 * The pixel is UNLIT iff it is void by the shade's rule, or a component of one of the three corner normals is not finite, or l is 0
 * or not finite.  An unlit pixel gets image = albedo EXACTLY (the background passes through, bit for bit), normal 0, shading 0.
 * There is no clamp: a negative s_c is stored as it is.  Light and albedo are plain IEEE.
 * THE BASIS is the UNNORMALISED polynomial one.  The irradiance of Ramamoorthi and Hanrahan ("An Efficient Representation for
 * Irradiance Environment Maps", 2001, eq. 13) with real-SH lighting coefficients L_lm and c1 = 0.429043, c2 = 0.511664, c3 = 0.743125,
 * c4 = 0.886227, c5 = 0.247708 (c3 = 3 c5) is this s with
 *   light[0] = c4 L_00,  light[1 .. 3] = 2 c2 (L_11, L_1-1, L_10),  light[4 .. 6] = 2 c1 (L_2-2, L_21, L_2-1),  light[7] = c1 L_22,
 *   light[8] = c5 L_20                                                  (c3 L_20 z^2 - c5 L_20 = c5 L_20 (3 z^2 - 1)).
 * CONTRACT, with u = 2^-24, eps = 2^-53, k_l = 16, k_c = 256 and per lit pixel c = sum_a w_a |n_a| / l >= 1 (how much the three
 * corner normals cancel; |.| the Euclidean norm), per channel:
 *   |image^_c - image_c| <= u |image_c| + k_l eps |albedo_c| sum_k |light_kc| |b_k| + k_c eps c |albedo_c| sum_{k >= 1} |light_kc|,
 * |shading^_c - s_c| the same without albedo, |normal^ - n| <= u + 32 eps c per component; the decision "lit" is exact unless l
 * underflows (|m| below 2^-500).
 * Derivation (every operation f64 and unfused).  w_a: 5 eps (the shade's).  A product w_a n_a: 6 eps; the two sums: |dm| <= 8 eps
 * sum_a w_a |n_a| per component, sqrt(3) times that in norm: 14 eps c l.  l: the squares, two sums and the root add 2.5 eps to the
 * 14 eps c l that dm moves it.  A component of n = m / l: 8 c + (14 c + 2.5) + 1 < 32 c eps (c >= 1).  b_k has a gradient of 1-norm
 * at most 6 on the unit ball (3 z^2 - 1) and at most 4 operations on magnitudes <= 3: |db_k| <= 6 x 32 c eps + 8 eps <= 200 c eps:
 * the third term, stated as k_c = 256 (b_0 = 1 is exact).  The sum: nine products and eight sums, then the product with albedo: 10 eps
 * sum |light b|, stated as k_l = 16.  The store rounds once: u |image|.
 * One thread per pixel, neighbouring lanes on neighbouring columns; a workgroup holds pixels of ONE frame, so the frame's light is
 * read at wave-uniform addresses (scalar loads), never gathered per lane.  Plain stores, no atomics, no workspace: bit-identical
 * from run to run, and a frame's outputs depend on that frame only.  Asynchronous on `stream`, no host synchronisation.
 * n_frames == 0: a successful no-op; n_faces == 0: image = albedo.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative
 * n_frames, n_channels outside 1 .. 4, a non-zero light stride below 9 n_channels, and with frames to write: NULL d_face / d_bary /
 * d_albedo / d_light / d_image, NULL d_verts or d_normals (n_faces > 0), a vertex or normal stride below 3 n_verts, 2^39 pixels or
 * more.                                                                                                                          */
int bodyfit_raster_light_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                long long verts_frame_stride, const float* d_normals, long long normals_frame_stride,
                                const float* d_albedo, int n_channels, const float* d_light, long long light_frame_stride,
                                int n_frames, float* d_image, float* d_normal /* may be NULL */, float* d_shading /* may be NULL */,
                                void* stream);
/* THE LIGHTING'S GRADIENTS (k_lt_grad, k_lt_light_sum, k_light.hip) for an upstream G = d_grad_image f32 [n_frames][H][W]
 * [n_channels]; the other inputs are bodyfit_raster_light_device's and the pixel is evaluated again by the same device function.
 * Three results, each skipped when its pointer is NULL:
 * (a) d_grad_albedo f32 [n_frames][H][W][n_channels]: G_c s_c on a lit pixel, G_c on an unlit one.
 * (b) d_grad_m f32 [n_frames][H][W][3]: the gradient in the UNNORMALISED interpolated normal m, what the rows VJP
 *     (bodyfit_surface_rows_vjp_device with the shade's weights) carries to the corner normals.  With t_c = G_c albedo_c, q_k = sum_c
 *     t_c light[k][c] (ascending c),  g_n = sum_k q_k grad b_k(n):
 *       g_x = ((q_1 + y q_4) + z q_5) + 2 x q_7,   g_y = ((q_2 + x q_4) + z q_6) - 2 y q_7,   g_z = ((q_3 + x q_5) + y q_6) + 6 z q_8,
 *     g_m = (g_n - n (n . g_n)) / l;  0 on an unlit pixel.
 * (c) d_grad_light f32 [n_frames][9][n_channels], ALWAYS per frame (a caller with a shared light adds the frames):
 *     g*[f][k][c] = sum over the lit pixels of frame f of t_c b_k(n).
 * HOW (c) IS SUMMED: a store pass and a fixed-order sum pass, no float atomics.  bodyfit_light_grad_layout (host only, no GPU) gives
 * the CHUNK: 256 P pixels, P the smallest power of two with at most 256 chunks per frame, at most 64: a function of H W only.  A
 * workgroup owns one chunk of one frame (chunks never straddle frames); thread j takes the pixels chunk + i 256 + j in ascending i
 * into its own f64 sums, the lanes of a wave are added by a butterfly (partners at distance 32, 16 .. 1: every lane holds the same
 * tree), the four waves in ascending order, and the chunk's [9][n_channels] f64 partial is stored into d_workspace, f64 [n_frames]
 * [n_chunks][9][n_channels] (*workspace_doubles of them; every one that is read is written first).  A second kernel adds a frame's
 * partials in ascending chunk order and rounds ONCE.  So d_grad_light is bit-identical from run to run, and a frame's 9 n_channels
 * numbers are a function of that frame's data and of (H, W, n_channels) only: not of n_frames, of the frame's place in the batch
 * or of the device's CU count.  A non-finite G or albedo on a lit pixel gives a non-finite coefficient in THAT frame only; an
 * unlit pixel adds nothing (it is skipped, not multiplied by 0).  1920 x 1080: P = 32, 254 chunks of 8,192 pixels.
 * CONTRACT, with u, eps, c, k_l, k_c of the lighting, k_m = 4096, k_r0 = 80, Q = sum_{k >= 1} sum_c |t_c light_kc|:
 *   (a) |ga^_c - ga_c| <= u |ga_c| + |G_c| (k_l eps sum_k |light_kc| |b_k| + k_c eps c sum_{k >= 1} |light_kc|) on a lit pixel; exact
 *       on an unlit one;
 *   (b) |gm^ - g_m| <= u |g_m| + k_m eps c Q / l per component;
 *   (c) |g^ - g*| <= u |g*| + eps sum over the frame's lit pixels of |t_c| ((k_r0 + n_chunks) |b_k| + k_c c).
 * Derivation.  (a): the lighting's, with G for albedo.  (b): |dn| <= 32 c eps per component; the second derivatives of the b_k are
 * at most 6 and a component of g_n has four terms: |dg_n| <= (18 x 32 c + 72) eps Q <= 650 c eps Q, |g_n| <= 10.4 Q in norm; the
 * projection: 2 x 1.8 x 32 c x 10.4 + 3 x 650 c < 3200 c eps Q; the division by l, which is 17 c eps off: 360 c eps Q more.  Together
 * below 4096 c eps Q / l.  (c): a term t_c b_k: two products and db_k <= k_c c eps; a sum of f64 numbers added along a path of at
 * most P + 6 + 3 + n_chunks <= 73 + n_chunks additions; the store's u.
 * One workgroup per chunk, plain stores.  Asynchronous on `stream`, NO host synchronisation and no allocation: the caller owns
 * d_workspace.  n_frames == 0, or all three outputs NULL: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): every
 * case of bodyfit_raster_light_device but d_image's, and with frames to write: NULL d_grad_image, d_grad_light without
 * d_workspace.  bodyfit_light_grad_layout: negative counts, n_channels outside 1 .. 4.
 * NOT BUILT: specular terms, shadows and ambient occlusion, SH orders above 2, the term's normal equations, the C++ mirror header's
 * entries.                                                                                                                      */
int bodyfit_light_grad_layout(long long pixels_per_frame, int n_channels, int n_frames, long long* chunk_pixels /* may be NULL */,
                              long long* n_chunks /* may be NULL */, long long* workspace_doubles /* may be NULL */);
int bodyfit_raster_light_grad_device(bodyfit_raster* r, const int32_t* d_face, const float* d_bary, const float* d_verts,
                                     long long verts_frame_stride, const float* d_normals, long long normals_frame_stride,
                                     const float* d_albedo, int n_channels, const float* d_light, long long light_frame_stride,
                                     int n_frames, const float* d_grad_image, float* d_grad_albedo /* may be NULL */,
                                     float* d_grad_m /* may be NULL */, float* d_grad_light /* may be NULL */,
                                     double* d_workspace /* may be NULL without d_grad_light */, void* stream);
/* SILHOUETTE-EDGE ANTIALIASING (k_rs_edges, k_rs_edge_blend, k_rs_edge_rows, k_raster_edges.hip): the coverage of a render as a smooth
 * function of the vertices, after Laine et al., "Modular Primitives for High-Performance Differentiable Rendering" (2020).  Only
 * COVERAGE carries a gradient here: how an attribute interpolates inside a face as its corners move is not part of it.
 * The handle keeps, per (face, edge e = corners e, (e + 1) % 3), the lowest-id OTHER face of the topology that holds both vertex ids
 * of the edge, -1 if none (or if the two ids are equal): 12 bytes per face, built by bodyfit_raster_create on the host.
 * DEFINITION, per frame, exact from the f32 vertices, the f64 intrinsics, z_near and cull_backfaces (projection and "drawn" are
 * those of bodyfit_raster_render_device), the images d_face int32 and d_depth f32 [H][W] of a render (a face value outside
 * [0, n_faces) is empty: it counts as -1 with depth +inf) and an image img f32 [H][W][C], C in 1 .. 4.
 * PAIRS.  Pixel p = (i, j) forms a pair with its right neighbour q = (i, j + 1) (axis 0) and with its lower neighbour q = (i + 1, j)
 * (axis 1).  A pair is a CANDIDATE iff face[p] != face[q].  The near pixel n is p if depth[p] <= depth[q], else q; o is the other;
 * t = face[n].  If t is empty or not drawn in this frame the pair does not blend.
 * CROSSING.  Axis 0: the scanline is y0 = i, the segment x in [j, j + 1], "along" is u and "across" is v; axis 1: y0 = j, the segment
 * v in [i, i + 1], along is v and across is u (exchange u and v throughout).  Written for axis 0, an edge (a, b) of a face CROSSES iff
 * exactly one of  v_a - y0 <= 0 < v_b - y0  and  v_b - y0 <= 0 < v_a - y0  holds (half-open: a vertex on the scanline counts once) and
 *   x* = u_a + (u_b - u_a) s,   s = (y0 - v_a) / (v_b - v_a),   lies in [j, j + 1], both ends included;   d = |x* - x_n|,
 * x_n the near pixel's centre on the segment (j or j + 1).
 * WALK.  Start in t with no entry edge; at most BODYFIT_AA_WALK = 8 steps (faces visited).  In each step: among the current face's
 * crossing edges other than its entry edge take the one of least d, ties to the lowest edge index; none: the pair does not blend.
 * Let t' be the table's face for that (face, edge).  The edge is a SILHOUETTE EDGE if t' does not exist, or t' is not drawn in this
 * frame (the cull flag counts), or t' is FOLDED over the current face: with side(x) = (u_b - u_a)(v_x - v_a) - (v_b - v_a)(u_x - u_a)
 * and c, c' the corners of the current face and of t' that are not on the edge, side(c) side(c') >= 0.  A silhouette edge ends the
 * walk: the pair BLENDS with (face, edge, s, x*, d).  Otherwise the walk steps into t' and the edge, identified by its two vertex ids,
 * becomes the entry edge.  Eight steps without a silhouette edge: the pair does not blend.  (Faces along a smooth silhouette are seen
 * edge-on and are thinner than a pixel: the face under the pixel centre is usually not the one that holds the silhouette edge, so the
 * walk is part of the definition.  On the two-sphere scene of the tests one face finds 120 of 242 body / background pairs, eight all.)
 * BLEND.  d >= 1/2: o receives alpha = d - 1/2 of (img[n] - img[o]); else n receives alpha = 1/2 - d of (img[o] - img[n]).
 * out[p] = img[p] + what p receives from its at most four pairs, taken in the order left, right, up, down.
 * WEIGHT IMAGE d_weight f32 [H][W][2], one entry per (pixel p, axis); a pair that would leave the image holds 0.  w > 0: q receives
 * w (img[p] - img[q]); w < 0: p receives |w| (img[q] - img[p]); w = 0: no blend.  |w| <= 1/2 always.
 * GRADIENT at the fixed images and walk.  With r the receiver and sigma = +1 if n = p, else -1:
 *   G = dL/dx* = sigma sum_c g[r][c] (img[n][c] - img[o][c]);
 * for axis 0, k = (u_b - u_a) / (v_b - v_a):  d(x*) / d(u_a, v_a) = (1 - s)(1, -k),  d(x*) / d(u_b, v_b) = s (1, -k);  with grad u = (fx / Z, 0,
 * -fx X / Z^2) and grad v = (0, fy / Z, -fy Y / Z^2) a blended pair is TWO rows of bodyfit_surface_rows_vjp_device:
 *   index = the walk's final face,  bary = one-hot at corner a | b,  coef = G (1 - s) | G s,  dir = m_a | m_b,  m = grad u - k grad v
 * at that corner (axis 1: m = grad v - k grad u, k = (v_b - v_a) / (u_b - u_a)).  The gradient in img is the blend's exact adjoint.
 * CONTRACT.  Every deciding operation is f64 and unfused, in this order: the projection of k_rs_faces; da = v_a - y0, db = v_b - y0;
 * den = v_b - v_a; s = (y0 - v_a) / den; x* = u_a + (u_b - u_a) s; d = |x* - x_n|; k = (u_b - u_a) / den; side as written above, the
 * fold test on the two signs; alpha = d - 1/2 or 1/2 - d.  Only stores round to f32.  No float atomics.  A frame's result depends on
 * that frame only: bit-identical from run to run and whatever n_frames.
 * BANDS, eps = 2^-53, P = P_t of the render's contract for the face at hand (for the fold test the larger of the two faces'), K =
 * |u_b - u_a| / |v_b - v_a| of the edge, k_c = 8, k_x = 32.  A decision is SURE when its quantity clears its band:
 *   area (drawn, culled):  |A| > 2^-46 P^2, the render's;      straddle:  |v_a - y0| >= tau_c = k_c eps P,  and v_b alike;
 *   inside the segment:  |x* - j|, |x* - (j + 1)| >= tau_x = k_x eps P (1 + K);    least d:  |d - d'| >= tau_x + tau_x';
 *   fold:  |side(c)|, |side(c')| >= 2^-46 P^2;             receiver:  |d - 1/2| >= tau_x;
 * and a decision whose f64 evaluation in the stated order is EXACT (it reproduces the exact value: every intermediate representable,
 * as on scenes with dyadic projections) is sure whatever its margin: the tie rules above then hold to the bit.  A candidate pair all
 * of whose decisions along the exact walk are sure is DECIDED.  For a decided pair, with w* the exact weight and u = 2^-24:
 *   |w - w*| <= u |w*| + 2 tau_x                                  (tau_x of the silhouette edge),
 * and for every pixel, with out* the exact blend of img by the RETURNED weights, T = |img[p]| + sum |w| |img[other] - img[p]| over the
 * amounts p receives, and k_b = 2:   |out - out*| <= k_b u T   (the adjoint alike, T = |g[p]| + sum |w| |g[p] or g[other]|); against the
 * exact weights add sum |w - w*| |img[other] - img[p]|.  A row pair of a decided pair, with k_r = 2, T_G = sum_c |g[r][c]| |img[n][c] -
 * img[o][c]|, tau_s = k_x eps P / |v_b - v_a|, tau_k = tau_s (1 + K), and M_c = |grad along|_c + |k| |grad across|_c at the corner:
 *   |coef - coef*| <= k_r u |coef*| + |G| tau_s + 2^-48 T_G,        |dir_c - dir*_c| <= k_r u M_c + tau_k |grad across|_c.
 * Derivation.  A projected coordinate is off by 3 eps P and a (coordinate - integer) by 4 eps P (the render's derivation): below tau_c.
 * den: two coordinates and a rounding, 8 eps P.  s in [0, 1]: (4 + 8 s) eps P / |den| + eps <= 13 eps P / |den|.  x*: 3 eps P from u_a,
 * 8 eps P s from u_b - u_a, |u_b - u_a| ds = 13 eps P K, the product's and the sum's roundings 3 eps P: below eps P (14 + 13 K) <= tau_x / 2;
 * x* - x_n and alpha round once each (2 eps) and the store once (u |w|), which gives the bound on w with room for the terms of second
 * order.  side: factors off by 8 eps P against partners <= 2 P, two products and a difference of numbers <= 4 P^2: 80 eps P^2 < 2^-46
 * P^2, as the render's area.  The blend: a difference of f32 in f64 (1 eps), a product, at most four sums: 7 eps T, and the store's u:
 * k_b = 2.  G: C products and sums, (C + 2) eps T_G <= 2^-50 T_G; (1 - s) and s carry ds <= tau_s / 2; the store u |coef|: k_r = 2.  k:
 * 8 eps P (1 + K) / |den| + eps K <= tau_k / 2; grad u, grad v: four roundings each, the store's u.
 * Shape: one thread per pixel, neighbouring lanes on neighbouring columns; equal ids cost two compares and one 8-byte store; only a
 * candidate pair gathers vertices and walks (a few per cent of the lanes).  Pairs across the render's tile borders are ordinary pairs.
 * bodyfit_raster_edges_device: d_verts as for the render, d_face / d_depth [n_frames][H][W] dense, d_weight f32 [n_frames][H][W][2]
 * dense, 8-byte aligned (it is read and written as pairs); every element is written, whatever it held.  Asynchronous on `stream`, no
 * host synchronisation, no workspace.  n_frames == 0:
 * a successful no-op; n_faces == 0: every weight 0.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames, z_near
 * <= 0 or NaN, fx or fy <= 0 or a non-finite intrinsic, and with frames to write: NULL d_weight, NULL d_verts / d_face / d_depth
 * (n_faces > 0), a stride below 3 n_verts, 2^39 pixels or more.                                                                   */
#define BODYFIT_AA_WALK 8
int bodyfit_raster_edges_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                const float* d_depth, float* d_weight, void* stream);
/* The blend of d_image f32 [n_frames][H][W][n_channels] by d_weight (as above), or with transpose != 0 its exact adjoint (d_image is
 * then the upstream gradient): d_out of the same shape, every element written; d_out must not be d_image.  One thread per pixel: it
 * gathers its four weights and neighbours and stores n_channels floats.  The topology is not used.  Asynchronous on `stream`.
 * n_frames == 0: a no-op.  BODYFIT_ERR_INVALID: NULL handle, negative n_frames, n_channels outside 1 .. 4, and with frames to write a
 * NULL d_weight / d_image / d_out, d_out == d_image, 2^39 pixels or more.                                                        */
int bodyfit_raster_edge_blend_device(bodyfit_raster* r, const float* d_weight, const float* d_image, int n_channels, int n_frames,
                                     int transpose, float* d_out, void* stream);
/* The ROWS of listed pairs (k_rs_edge_rows): d_pair int32 [N] = 2 (i W + j) + axis inside the pair's frame, d_offset int32
 * [n_frames + 1] the ragged convention of the depth rows, or NULL: N / n_frames pairs per frame.  d_image and d_grad f32
 * [n_frames][H][W][n_channels]: the blended image's input and the upstream gradient of its output.  The kernel repeats the walk and
 * writes rows 2 n (corner a) and 2 n + 1 (corner b) of pair n: d_index int32 [2 N], d_bary f32 [2 N][3], d_coef f32 [2 N], d_dir f32
 * [2 N][3]; a listed pair that does not blend (or lies outside the image) gets index -1, bary = dir = 0 and coef = 0.  Every row is
 * written.  The rows' frame structure for bodyfit_surface_rows_vjp_device is 2 d_offset.  Asynchronous on `stream`, no workspace.
 * n_frames == 0 or N == 0: a no-op; n_faces == 0: every row void.  BODYFIT_ERR_INVALID: NULL handle, negative counts, n_channels
 * outside 1 .. 4, z_near <= 0 or NaN, fx or fy <= 0 or a non-finite intrinsic, pairs without frames, a uniform N that n_frames does not
 * divide, 2^30 pairs or pixels of a frame or more, and with rows to write: NULL d_pair or output, NULL d_verts / d_face / d_depth /
 * d_image / d_grad (n_faces > 0), a stride below 3 n_verts.                                                                      */
int bodyfit_raster_edge_rows_device(bodyfit_raster* r, const float* d_verts, long long verts_frame_stride, int n_frames, double fx,
                                    double fy, double cx, double cy, float z_near, int cull_backfaces, const int32_t* d_face,
                                    const float* d_depth, const float* d_image, const float* d_grad, int n_channels,
                                    const int32_t* d_pair, const int32_t* d_offset /* may be NULL */, long long n_pairs,
                                    int32_t* d_index, float* d_bary, float* d_coef, float* d_dir, void* stream);
/* Statistics of the handle's latest render (from its read-back; no synchronisation): the (face, tile) pairs binned, and the
 * longest tile list.                                                                                                          */
int bodyfit_raster_last_bins(bodyfit_raster* r, long long* n_entries, int* longest);

/* SIGNED-DISTANCE VOLUMES (k_vol_sample, k_volume.hip; the host side: api_volume.hip): a scalar volume read trilinearly at the
 * points of a cloud, with the exact spatial gradient there: the 3-D counterpart of bodyfit_raster_sample_device.  It is what a body
 * is measured against when the world around it is given as a distance field: a pre-scanned scene, a fused TSDF, an object.
 * The handle holds the GEOMETRY only, as the raster handle holds an image size: nx, ny, nz >= 1 voxels with nx ny nz < 2^31, the
 * position `origin` of voxel (0, 0, 0) and the `spacing` between voxels per axis (finite; spacing > 0; the axes may differ).  It
 * owns no device memory and no workspace: calls on one handle need no ordering.  BODYFIT_ERR_INVALID: NULL out / origin / spacing,
 * a dimension below 1, 2^31 voxels or more, a non-finite origin, a spacing that is not finite and positive or whose reciprocal is
 * not a normal f64 number.                                                                                                       */
typedef struct bodyfit_volume bodyfit_volume;
int bodyfit_volume_create(int device, int nx, int ny, int nz, const double origin[3], const double spacing[3],
                          bodyfit_volume** out);
void bodyfit_volume_destroy(bodyfit_volume* h);
/* d_points f32 [n_frames][n_points][3], points_frame_stride floats between frames (>= 3 n_points: bodyfit_device_views.cloud is
 * used in place).  d_volume f32 [nz][ny][nx], x fastest; volume_frame_stride ELEMENTS between the frames' volumes: 0 when the frames
 * share one, else >= nx ny nz.  d_gate u8 [n_frames][n_points] or NULL.  Outputs d_value f32 [n_frames][n_points], d_valid u8
 * [n_frames][n_points] and, unless NULL, d_grad f32 [n_frames][n_points][3] = (d/dx, d/dy, d/dz) in WORLD units (value per metre
 * when the points are metres).  Every element is written; a dead point gets 0 everywhere and valid 0.
 * DEFINITION.  Voxel (k, j, i) sits at origin + (i sx, j sy, k sz).  Grid coordinates g = (p - origin) / spacing, per axis, in f64.
 * A point is LIVE iff its coordinates are finite, its gate byte is non-zero (or d_gate is NULL), 0 <= g_a <= n_a - 1 on every axis,
 * and ALL EIGHT VOXELS OF ITS CELL ARE FINITE: a TSDF marks unobserved space with NaN or inf, and a vertex there costs nothing
 * rather than poison a sum.  The cell is bilinear_cell's on three axes: i0 = min(floor(gx), max(nx - 2, 0)), i1 = min(i0 + 1,
 * nx - 1), a = gx - i0, and (j0, j1, b) in y, (k0, k1, c) in z alike.  With V[dk][dj][di] = volume[k_dk][j_dj][i_di],
 *   value = sum over (dk, dj, di) of  (di ? a : 1 - a) (dj ? b : 1 - b) (dk ? c : 1 - c) V[dk][dj][di],
 *   d/dx  = ((1-b)(1-c) (V001 - V000) + b (1-c) (V011 - V010) + (1-b) c (V101 - V100) + b c (V111 - V110)) / sx,
 *   d/dy  = ((1-a)(1-c) (V010 - V000) + a (1-c) (V011 - V001) + (1-a) c (V110 - V100) + a c (V111 - V101)) / sy,
 *   d/dz  = ((1-a)(1-b) (V100 - V000) + a (1-b) (V101 - V001) + (1-a) b (V110 - V010) + a b (V111 - V011)) / sz:
 * the exact derivative of the trilinear patch of the cell, over the spacing (at g_a = n_a - 1 the last cell's, taken from inside;
 * an axis of length 1 has i1 = i0: derivative 0).
 * CONTRACT, with u = 2^-24, E = max(nx, ny, nz), delta = 2^-50 E (in voxels) and M the largest |voxel| among the voxels of the
 * exact cell and of the returned cell:
 *   (a) a point that passes the other tests and lies at least delta inside the box [0, n_a - 1]^3 is tested on the voxels of a cell
 *       K whose closed support is within delta of the exact g, and is live iff K's eight are finite; a point returned live lies
 *       within delta of the box; the tests on the gate and on finiteness (of the point, of K's voxels) are exact, and so is
 *       g_a = 0 for a coordinate that equals the origin's (the only way onto an axis of length 1);
 *   (b) |value^ - T(g)| <= u |T| + 2^-46 E M, T the continuous piecewise-trilinear field through the voxels (where the exact
 *       cell holds a voxel that is not finite and K does not: K's patch, extended);
 *   (c) each returned derivative is within u |g_K| + 2^-46 E M / spacing of the derivative g_K of K's patch at g, K the cell of (a).
 * Derivation (eps = 2^-53; every operation f64 and unfused).  g^: an f32 coordinate is exact in f64; the kernel multiplies by
 * 1 / spacing, formed once on the host, where the definition divides: the reciprocal, the difference and the product round once
 * each, 3 eps |g| (1 + eps)^2 < 2^-51 E for a point within delta of the box: inside delta.  The comparisons and
 * floor act on g^, which gives (a), and the returned cell K holds g^ in its closed support.  a = g^ - i0 is exact (Sterbenz, or
 * i0 = 0 and a = g^).  T is continuous and, inside a cell, of slope at most 2 M per voxel in each coordinate.  Let c be g clamped
 * onto K's closed support: c lies in the exact cell too, within delta of g per axis, and within delta of g^: |T(g) - T(c)| <= 6 M
 * delta in the exact cell and |T(c) - T(g^)| <= 6 M delta in K, together 12 M delta < 2^-46.4 E M.  The patch evaluated in f64:
 * three 1 - x, two products per weight, one product with the voxel, three levels of sums: below 16 eps M = 2^-49 M.  Together
 * below 2^-46 E M; the store rounds once: u |T|.  A derivative of K's patch in grid units is bilinear in the other two
 * coordinates with slope at most 4 M in each: 8 M delta = 2^-47 E M for the move from g to g^; a difference of two voxels rounds
 * once, two products, two levels of sums: below 16 eps M; the product with 1 / spacing twice more: 2 eps (2 M).  Over the spacing,
 * together below 2^-46 E M / spacing; the store's u |g_K|.  (A result below 2^-126 in magnitude is stored to a multiple of 2^-149:
 * with M below 2^-100 the statement lacks that term.)
 * One thread per (frame, point); the eight voxels are gathered before anything is combined.  Plain stores, no atomics, no
 * workspace: bit-identical from run to run, a frame's outputs depend on that frame only (bit-identical whatever n_frames), and
 * d_value / d_valid do not depend on whether d_grad is given.  Asynchronous on `stream`, no host synchronisation.  n_frames == 0 or
 * n_points == 0: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle, negative n_frames or n_points, and
 * with points to write: NULL d_points / d_volume / d_value / d_valid, a point stride below 3 n_points, a volume stride that is
 * neither 0 nor >= nx ny nz, 2^39 points or more.
 * NOT BUILT: the gradient in the voxels, multi-channel volumes, i16 / f16 storage, extrapolation outside the volume, and the
 * entries of the C++ mirror header.                                                                                             */
int bodyfit_volume_sample_device(bodyfit_volume* h, const float* d_points, long long points_frame_stride, long long n_points,
                                 int n_frames, const float* d_volume, long long volume_frame_stride,
                                 const uint8_t* d_gate /* may be NULL */, float* d_value, uint8_t* d_valid,
                                 float* d_grad /* may be NULL */, void* stream);
/* TSDF FUSION (k_tsdf_integrate, k_tsdf.hip): depth maps integrated into a truncated signed-distance volume of the handle's
 * geometry, the volume that bodyfit_volume_sample_device reads.  d_depth f32 [n_frames][height][width] metres ALONG THE OPTICAL
 * AXIS (the depth of bodyfit_raster_render_device and of the depth terms), depth_frame_stride floats between frames (>= height
 * width); intr = (fx, fy, cx, cy), pixel (i, j) at (u, v) = (j, i); d_pose f64 [n_frames][12], row-major [A | t], world -> camera,
 * or NULL: the identity (orthonormality is not checked: the definition is in q = A p + t).  d_tsdf / d_weight f32 [nz][ny][nx]:
 * volume_frame_stride 0: every frame is fused into ONE volume, in ascending order; >= nx ny nz: frame f goes into volume f alone
 * (the per-frame distance volumes of a moving subject).  reset != 0: the buffers' contents are ignored, the start state is empty.
 * DEFINITION.  The state of a voxel is (D, W): D the truncated signed distance in metres, POSITIVE in front of the surface (the
 * sign of a voxelised scene), W the weight.  A voxel is OBSERVED iff W > 0 and D is finite; any other state, whatever its bits,
 * is unobserved, and an unobserved voxel is written as (NaN, 0): the sampler's dead voxel.  With p = origin + (i sx, j sy, k sz)
 * and q = A p + t, frame f updates the voxel iff ALL of (each false on a NaN)
 *   1. q_z > z_near;
 *   2. with u = fx q_x / q_z + cx, v = fy q_y / q_z + cy, the nearest pixel (i, j) = (floor(v + 1/2), floor(u + 1/2)) has
 *      0 <= i <= height - 1 and 0 <= j <= width - 1 (tested on the f64 values);
 *   3. d = depth[f][i][j] is finite and d > 0 (a pixel that holds nothing: 0, negative, NaN, inf);
 *   4. s = d - q_z >= -trunc (otherwise the voxel is hidden behind the surface and stays as it was).
 * Then, with sb = min(s, trunc) and (W, W D) = (0, 0) for an unobserved voxel:
 *   D' = f32((W D + sb) / (W + 1)),   W' = f32(min(W + 1, max_weight)),
 * each rounded to f32 ONCE PER FRAME, which makes a call with n frames BIT-IDENTICAL to n calls with one frame each and to any
 * split into consecutive calls that carry (D, W); with a cap the average depends on the order, so the order is part of it.
 * CONTRACT, with u = 2^-24, eps = 2^-53 and, per voxel and frame, P_a = |origin_a| + index_a s_a, S_r = sum_c |A_rc| P_c + |t_r|
 * (S_r = P_r without a pose), dd = min(d, 2 (S_z + trunc)):
 *   (a) decision 1 is exact unless |q_z - z_near| <= 2^-50 S_z, decision 4 unless |s + trunc| <= delta_4 = 2^-50 (S_z + dd);
 *   (b) for q_z >= 2^-40 S_z each pixel index is floor(x + 1/2 + e) for some |e| <= delta_p(x), x = u or v,
 *       delta_p(u) = 2^-49 (|fx| (S_x + |q_x / q_z| S_z) / q_z + |u| + |cx| + 1) pixels (v: fy, S_y, q_y, cy); the range test and
 *       decision 3 are exact for that pixel; for a smaller q_z that passes decision 1 the pixel is not constrained;
 *   (c) W' is exact, and so is an untouched voxel's state; with D'* the definition's value for SOME decision vector (and pixel)
 *       admissible under (a) and (b),  |D' - D'*| <= u |D'*| + delta_4 / (W + 1) + 2^-50 (|D| + |sb|) + 2^-149.
 * Derivation (every operation f64 and unfused; only the two stores round to f32).  p^: a product and a sum, 2 eps P_a.  q^: three
 * products and three sums, the first term through four roundings, plus |A| carried over p^'s error: below 6.5 eps S_r < 2^-50
 * S_r, which is (a) for decision 1.  s^ = d - q^_z (d is exact in f64) rounds once more: 6.5 eps S_z + eps (d + S_z) <= 2^-50
 * (S_z + d); for d > 2 (S_z + trunc) both s and s^ exceed trunc: the decision and sb = trunc are exact, whence dd.  The kernel
 * forms 1 / q^_z once and multiplies where the definition divides: for q_z >= 2^-40 S_z the move from q to q^ changes fx q_x / q_z
 * by at most 1.001 x 6.5 eps |fx| (S_x + |q_x / q_z| S_z) / q_z; the product, the reciprocal, the second product, the sum with cx
 * and the sum with 1/2 round once each: 5 eps |u| + 3 eps |cx| + eps / 2; together below 7 eps (...) < delta_p.  The average:
 * the product W D, the sum, W + 1 (exact below 2^53) and the quotient: 4 eps |D| + 3 eps |sb| beside sb's own error over W + 1; the
 * store rounds once, u |D'*|, to a multiple of 2^-149 below 2^-126.
 * One lane per voxel, x fastest; the state is read at most once (not under reset), kept in registers over the frames and written
 * once; a frame's camera is wave-uniform; the depth gathers of several frames are issued ahead of their use.  Plain stores, no
 * atomics, no workspace: bit-identical from run to run.  Asynchronous on `stream`, no host synchronisation, no allocation.
 * n_frames == 0 launches nothing, unless reset != 0 and volume_frame_stride == 0: then the empty state is written.
 * BODYFIT_ERR_INVALID (nothing is launched): NULL handle; n_frames < 0; height or width below 1; height width >= 2^31; a depth
 * stride below height width; a volume stride that is neither 0 nor >= nx ny nz; trunc not finite or not > 0; z_near not finite or
 * < 0; max_weight not > 0 (+inf: no cap); NULL intr, an intrinsic that is not finite, fx or fy zero; with work to do: NULL
 * d_tsdf / d_weight, NULL d_depth with frames to fuse, 2^31 workgroups (256 voxels each, per volume) or more.
 * NOT BUILT: the Euclidean ray length as the measure, a bilinear depth lookup, per-pixel weights, colour volumes, the gradient
 * in the voxels, and the entry of the C++ mirror header.                                                                       */
int bodyfit_volume_integrate_device(bodyfit_volume* h, const float* d_depth, long long depth_frame_stride, int height, int width,
                                    int n_frames, const double intr[4], const double* d_pose /* [n_frames][12] or NULL */,
                                    double trunc, double z_near, double max_weight, int reset, float* d_tsdf, float* d_weight,
                                    long long volume_frame_stride, void* stream);
/* SURFACE EXTRACTION (k_mc_*, k_surface_extract.hip): the level set value = iso of a volume of the handle's geometry as a welded
 * triangle mesh, marching cubes: what turns a fused TSDF or a voxelised scene back into the vertices and faces that the mesh
 * entries take (bodyfit_raster_render_device, bodyfit_surface_*).  d_volume f32 [nz][ny][nx], or n_volumes of them
 * volume_frame_stride ELEMENTS apart (>= nx ny nz; or 0, the sampler's shared volume: every one of the n_volumes is the same);
 * d_weight the same shape and stride, or NULL.
 * DEFINITION.  A voxel is USABLE iff its value is finite and (d_weight is NULL or its weight >= min_weight: false on a NaN
 * weight).  It is INSIDE iff value < iso, compared exactly on the f32 values: -0.0 and a value equal to iso are outside.  A CELL
 * (k, j, i), 0 <= i <= nx - 2 and alike in j and k (an axis of length 1 has no cells: the result is empty), has the corners
 * c = 0 .. 7 at (i + (c & 1), j + (c >> 1 & 1), k + (c >> 2 & 1)); it is LIVE iff all eight are usable (the sampler's rule for a
 * dead cell), and its CASE is the 8-bit number whose bit c is set iff corner c is inside.
 * THE TABLE (csrc/mc_table_inl.h, WRITTEN BY tools/gen_mc_table.py from this rule; it is part of the definition).  Cube edge
 * e = 4 axis + r joins the r-th corner (ascending) whose `axis` bit is clear to that corner with the bit set: axis 0: (0,1) (2,3)
 * (4,5) (6,7); axis 1: (0,2) (1,3) (4,6) (5,7); axis 2: (0,4) (1,5) (2,6) (3,7).  On each of the six cube faces the crossed face
 * edges are joined by segments: two crossings, one segment; four crossings (the ambiguous face), two segments that each cut off ONE
 * INSIDE corner, so inside corners are separated; the two cells that share a face see the same four signs and draw the same
 * segments.  Every segment is directed with one handedness (seen from outside the cube, the inside corners it cuts off lie on its
 * right), which makes case 1 (corner 0 alone inside) the triangle (0, 4, 8), its normal away from corner 0: normals point towards
 * INCREASING values, outward for a voxelised mesh (negative inside), towards the sensor for a TSDF.  A crossed edge lies on two
 * faces and so has one segment in and one out: following them closes loops, taken in ascending order of their smallest edge, each
 * from that edge in its direction.  A loop of length L gives the fan of L - 2 triangles (a, v_m, v_m+1), m = 1 .. L - 2, from an
 * apex a = v_0: the first rotation of the loop none of whose fan diagonals (a, v_m), 2 <= m <= L - 2, joins two edges of one cube
 * face: such a diagonal would lie in that face and coincide with a diagonal or a segment of the neighbouring cell there, an edge
 * used by more than two triangles.  (Derived, not recalled: every case has an apex; 820 triangles in all, at most 5 in a row,
 * 2 / 16 / 50 / 80 / 76 / 32 rows with 0 .. 5; because the segments on a shared face agree and are traversed in opposite
 * directions by the two cells, every interior triangle edge is used once in each direction: the mesh is a closed oriented manifold
 * wherever no dead cell and no border of the volume cuts it.  tests/test_extract.py checks all of it.)
 * VERTICES (welded).  Voxel (k, j, i) OWNS the three grid edges that leave it towards +x, +y, +z.  An owned edge carries a vertex
 * iff both ends are usable, exactly one end is inside AND at least one of the up to four cells around the edge is live: no vertex
 * is unreferenced.  Order: ascending linear index (k ny + j) nx + i of the owner, then x, y, z within an owner.  Position, with a
 * the owner, b the neighbour and t = (iso - V_a) / (V_b - V_a) (0 <= t <= 1): origin + (index + t) spacing along the edge, origin
 * + index spacing on the other two axes.
 * FACES.  A live cell emits its case's triangles in table order, the cells in ascending linear index of their corner 0; a corner is
 * the index of the vertex on that cube edge, int32, LOCAL to its volume.  Zero-area triangles (a value equal to iso: t = 0) are
 * kept: the topology stays manifold, and bodyfit_surface_closest_device defines degenerate faces.
 * bodyfit_volume_surface_layout: the bytes of the workspace that the two device entries share for n_volumes volumes (3 bytes per
 * voxel and 8 per 256 voxels, rounded up).  bodyfit_volume_surface_count_device: d_offsets i64 [2][n_volumes + 1], the exclusive
 * vertex offsets of the volumes, then their face offsets; the last of each is the total.  bodyfit_volume_surface_emit_device, with
 * THE SAME inputs, workspace and offsets (the caller reads the totals, allocates and must not change the volume in between; emit
 * reads the volume again for the positions): d_verts f32 [vert_capacity][3], volume f's at offsets[0][f]; d_faces i32
 * [face_capacity][3], volume f's at offsets[1][f].  EVERY STORE IS GUARDED by the capacities: a caller that passes less than the
 * totals gets the leading part of the mesh and no write past its buffers.
 * CONTRACT, with u = 2^-24 and eps = 2^-53: the offsets, the totals and every face index are EXACT.  The coordinate along the edge
 * satisfies |x^ - x*| <= u |x*| + 2^-50 (|origin_a| + (index + 1) s_a) + 2^-149; the other two are within u |x*| + 2^-51
 * (|origin_a| + index s_a) + 2^-149.  Derivation (every operation f64 and unfused, one store to f32): an f32 value is exact in
 * f64; iso - V_a, V_b - V_a and their quotient round once each, and rounding is monotone, so t^ stays in [0, 1] and |t^ - t| <=
 * 3.01 eps; index + t^ rounds once, eps (index + 1); the product with s_a once, eps (index + 1) s_a; the sum with the origin once,
 * eps (|origin_a| + (index + 1) s_a): together below 6.1 eps (|origin_a| + (index + 1) s_a) < 2^-50 (...).  Off the edge: a product
 * and a sum, 2 eps (...) = 2^-52 (...), stated as 2^-51.  The store rounds once, u |x*|, to a multiple of 2^-149 below 2^-126.
 * Five launches: per voxel a byte (its cell's case, 0 when dead) and a u16 (its edge flags over its vertex offset inside the
 * workgroup), a scan of the workgroup sums per volume, a scan over the volumes, the emit.  Integer sums in a fixed order, plain
 * stores, no atomics: bit-identical from run to run, and a volume's mesh is bit-identical whatever n_volumes and its place in the
 * batch.  Asynchronous on `stream`; no host synchronisation, no allocation; the handle still owns no device memory.
 * n_volumes == 0: nothing is launched and the two zero offsets are written (when d_offsets is given); an axis of length 1: nothing
 * is launched and the offsets are zeroed.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle; n_volumes < 0; a volume stride
 * that is neither 0 nor >= nx ny nz; iso not finite; min_weight NaN; a geometry that could hold 2^31 vertices or faces of one volume
 * or more (3 nx ny nz or 5 (nx - 1)(ny - 1)(nz - 1) >= 2^31); with volumes: NULL d_offsets, and with cells: NULL d_volume or
 * d_workspace, 2^31 workgroups (256 voxels each, per volume) or more; emit: a negative capacity, NULL d_verts or d_faces with a
 * capacity above 0 (both capacities 0: a successful no-op).
 * NOT BUILT: vertex normals or colours from the volume, the gradient of the vertices in the voxels, decimation, a capacity-only
 * single call without the host's read of the totals, and the entries of the C++ mirror header.                                 */
int bodyfit_volume_surface_layout(bodyfit_volume* h, int n_volumes, long long* workspace_bytes);
int bodyfit_volume_surface_count_device(bodyfit_volume* h, const float* d_volume, const float* d_weight /* may be NULL */,
                                        long long volume_frame_stride, int n_volumes, float iso, float min_weight,
                                        void* d_workspace, long long* d_offsets /* i64 [2][n_volumes + 1] */, void* stream);
int bodyfit_volume_surface_emit_device(bodyfit_volume* h, const float* d_volume, const float* d_weight /* may be NULL */,
                                       long long volume_frame_stride, int n_volumes, float iso, float min_weight,
                                       void* d_workspace, const long long* d_offsets, long long vert_capacity,
                                       long long face_capacity, float* d_verts, int32_t* d_faces, void* stream);
/* VOLUME DISTANCE TRANSFORM with the nearest seed (a 3-D feature transform) of n_volumes masks of the handle's dims (k_edt3.hip over
 * k_edt.hip): a full distance field from a mask (a visual hull, a segmented scan) or from the crossings of a TSDF, where the TSDF
 * itself is a distance only inside its band.  The seed kinds are those of bodyfit_raster_distance_device: seed_kind 0, d_seed is
 * u8 [n_volumes][nz][ny][nx] and a voxel is a SEED iff its byte is != 0; seed_kind 1, int32 and a seed iff its value is >= 0.
 * seed_volume_stride elements (bytes or int32) between volumes, >= nx ny nz.  invert != 0 swaps seeds and non-seeds.  Outputs
 * d_dist2 and, unless NULL, d_nearest: int32 [n_volumes][nz][ny][nx], dense, volume after volume.
 * DEFINITION, exact, in integers and in INDEX units (the handle's spacing and origin are not used), for voxel (k, j, i) of volume v:
 *   dist2[v][k][j][i]   = min over the seeds (k', j', i') of volume v of (k - k')^2 + (j - j')^2 + (i - i')^2,
 *   nearest[v][k][j][i] = (k' ny + j') nx + i' of a seed that ATTAINS that minimum.
 * A seed voxel has dist2 0 and nearest itself.  A volume without a seed gets dist2 = INT32_MAX and nearest = -1 at every voxel.
 * Range: EVERY DIMENSION IS AT MOST 16384 (a larger one: BODYFIT_ERR_INVALID), so dist2 <= 3 x 16383^2 < 2^30; g below is a 2-D
 * dist2 <= 2 x 16383^2 < 2^29, a squared slice difference is < 2^28, so each side of the comparison below is < 2^28 + 2^29 < 2^30
 * and the numerator of the division is |u^2 - s^2| + |g_u - g_s| < 2^28 + 2^29 < 2^30 in magnitude: int32 throughout.
 * TIE RULE.  Among the seeds at the minimum the choice is a fixed function of the volume's mask: inside a slice the rule of
 * bodyfit_raster_distance_device; along z the slice that entered the lower envelope first keeps every voxel at which a later
 * slice only equals it.  So nearest is always the same one, but it is not "the lowest index": use it as A nearest seed.
 * CONTRACT.  No tolerance: dist2 equals the definition at every voxel, and nearest is a seed of the same volume at exactly that
 * squared distance.  Every output element is written, whatever the outputs held.  No atomics, plain stores: bit-identical from run
 * to run, and a volume's outputs depend on that volume only (identical whatever n_volumes and the stride).
 * Derivation.  Stage xy is the 2-D transform of each slice k (a frame of W = nx, H = ny): d2(k, j, i), the minimum over the seeds
 * of slice k alone, INT32_MAX in a slice without a seed, and n2 = j' nx + i'.  Then dist2(x, j, i) = min_k F_k(x), F_k(x) =
 * (x - k)^2 + d2(k, j, i) over the slices that have a seed: the column pass of the 2-D transform with an ARBITRARY g_k = d2(k),
 * the same exact comparison F_s(t_s) <= F_u(t_s), the same true floor division for the first slice t_u at which u is strictly
 * better, exact for the reason given there (an integer is <= a rational iff it is <= its floor).  Because g_s cannot be
 * recomputed from the payload and is needed after slice s itself has been written on the way back (the reigning slice may lie
 * above the voxel), the z pass does NOT run in place: g_s travels in the stack entry, d2 and n2 are read-only and the outputs are
 * separate arrays.
 * Shape: k_edt_rows and k_edt_cols unchanged over the n_volumes nz slices; k_edt_depth one lane per (volume, j, i) column,
 * neighbouring lanes on neighbouring i.  bodyfit_volume_distance_layout: the bytes of the workspace for n_volumes volumes, 16 per
 * voxel of a group (the stack that both stages share, d2, n2); a batch of more than 2^28 voxels is worked group after group
 * of whole volumes on the stream, so the workspace stays at 4 GiB unless one volume alone is larger.  d_workspace is 8-byte
 * aligned.  Asynchronous on `stream`, no host synchronisation, no allocation: the handle still owns no device memory.  n_volumes
 * == 0: a successful no-op.  BODYFIT_ERR_INVALID (nothing is launched): NULL handle; negative n_volumes; a dimension above 16384;
 * seed_kind not 0 or 1; layout: NULL workspace_bytes; with volumes to write: NULL d_seed / d_dist2 / d_workspace, a workspace that
 * is not 8-byte aligned, a stride below nx ny nz.
 * NOT BUILT: anisotropic metrics, sub-voxel seed positions, gradients of the transform, the entries of the C++ mirror header.   */
int bodyfit_volume_distance_layout(bodyfit_volume* h, int n_volumes, long long* workspace_bytes);
int bodyfit_volume_distance_device(bodyfit_volume* h, const void* d_seed, int seed_kind, long long seed_volume_stride,
                                   int n_volumes, int invert, void* d_workspace, int32_t* d_dist2,
                                   int32_t* d_nearest /* may be NULL */, void* stream);

/* kernels launched by this process through the library so far (benchmarks: launches per LM iteration) */
long bodyfit_launch_count(void);
const char* bodyfit_last_error(void);
int bodyfit_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* BODYFIT_H_ */
