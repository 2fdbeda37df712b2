/*
 * pfmpe.h — C-ABI of the MI355X particle-filter pose engine (the drop-in boundary).
 *
 * The reference has no function/plugin boundary around its PF step: the step is ~200 inline lines in
 * PoseEstimator::estimateBodyPose (pf_mpe_lib/src/pose_estimator.cpp:475-733, "PE" below) sharing ~15
 * member fields (pf_mpe_lib/include/pf_mpe_lib/pose_estimator.h:65-169).  This header cuts it at the
 * PE:535 seam: the host keeps detection, prediction (predictPose PE:995), initialisation and Gauss-Newton
 * (PE:1805) and replaces PE:475-733 with one pfmpe_step() call.  Each entry point below cites the
 * reference state or code it replaces.  Plain C types only — no HIP/torch types cross the boundary.
 *
 * Conventions
 *   - Poses are 12 doubles: the top 3 rows of the homogeneous 4x4, row-major:
 *       [r00 r01 r02 t0  r10 r11 r12 t1  r20 r21 r22 t2]   (the Eigen::Matrix4d of the reference).
 *   - Blob coordinates are undistorted pixels (image_points_, PE:469 / led_detector.cpp:198-209), B x 2.
 *   - Return codes: 0 = OK, < 0 = error (PFMPE_E_*); pfmpe_last_error() gives text.  Algorithmic
 *     outcomes (accept / re-initialise) are NOT errors: see pfmpe_frame_out.flag_fail (reference codes).
 *   - A context is bound to one HIP device and one HIP stream and is not thread-safe; distinct contexts
 *     share nothing and may run concurrently (one per camera stream / tracked object / GPU).
 *   - pfmpe_step() is blocking: it returns after the frame's scalars and winner pose are on the host.
 *     The resampled particle set stays resident in HBM across frames (newPoseEstimation, PE:681).
 */
#ifndef PFMPE_H_
#define PFMPE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PFMPE_ABI_VERSION 1
#define PFMPE_MAX_MARKERS 16   /* reference bMarkerDowngrade has 5 entries; we take per-marker flags */
#define PFMPE_MAX_BLOBS 1024

enum {
  PFMPE_OK = 0,
  PFMPE_E_ARG = -1,   /* bad argument / size                      */
  PFMPE_E_HIP = -2,   /* HIP runtime failure (device, alloc, launch) */
  PFMPE_E_CAP = -3,   /* exceeds the capacity given at create time  */
  PFMPE_E_STATE = -4  /* call order (e.g. step before set_model)    */
};

/* particle state storage in HBM (SoA planes).  F16: fp16 deltas to an anchor pose per particle set
 * (the frame's current pose for a resampled set, the first particle for pfmpe_set_prior), fp32 compute
 * and fp32 weights: 24 B per particle (BASELINE.json configs[3]), stored as 6 planes of fp16 pairs.  The
 * layout is internal: every entry point exchanges poses as 12 doubles per particle. */
enum { PFMPE_STATE_F32 = 0, PFMPE_STATE_F64 = 1, PFMPE_STATE_F16 = 2 };

/* motion / resample random streams */
enum {
  PFMPE_RNG_REFERENCE = 0, /* std::default_random_engine (minstd_rand0) stream of PE:476-477, 510-523,
                              reproduced on device by LCG jump-ahead: bit-identical draws */
  PFMPE_RNG_PHILOX = 1     /* counter-based Philox4x32-10 keyed by (seed, frame, iter, particle) */
};

/* flag_fail codes (pf_mpe/include/pf_mpe/monocular_pose_estimator.h:121-137, PE:635, PE:711) */
enum { PFMPE_FLAG_ACCEPTED = 1, PFMPE_FLAG_REINIT = 4 };

typedef struct pfmpe_ctx pfmpe_ctx;

/* PF parameters — the public fields of PoseEstimator (pose_estimator.h:121-155) that the PF block reads,
 * plus the constants the reference hard-codes (made explicit, defaults = reference values). */
typedef struct {
  double tol;        /* back_projection_pixel_tolerance_   score normaliser (PE:2416)           */
  double tol_pf;     /* back_projection_pixel_tolerance_PF acceptance gate (PE:2414)            */
  double ang_min;    /* minAngularNoise   (rad)                                                 */
  double ang_max;    /* maxAngularNoise   (rad)                                                 */
  double trans_min;  /* minTransitionNoise (m)                                                  */
  double trans_max;  /* maxTransitionNoise (m)                                                  */
  double growth;     /* 0.025: noise growth per 10 iterations (PE:563)                          */
  int32_t max_iter;  /* 80  (PE:616)                                                            */
  int32_t exit_cap;  /* 5   exit when max w >= M*min(exit_cap, B)   (PE:616)                    */
  int32_t accept_cap;/* 3   accept when best > M*min(accept_cap, B) (PE:633)                    */
  int32_t rng_mode;  /* PFMPE_RNG_*                                                             */
} pfmpe_params;

/* Per-frame host inputs */
typedef struct {
  double current_pose[12];   /* current_pose_   -> particle 0 (PE:547)                          */
  double predicted_pose[12]; /* camMoveInv * predicted_pose_ (PE:395) -> particle 1 (PE:551)    */
  double prediction[12];     /* predictionMatrix = predictPose() (PE:234, PE:995-1010)          */
  double cam_move_inv[12];   /* camMoveInv (identity unless bUseCamPos, PE:241-393)             */
  const double* blobs;       /* B x 2 undistorted px; host pointer (ignored if bank_frame >= 0)  */
  int32_t B;                 /* numLED (PE:449)                                                 */
  int32_t bank_frame;        /* -1: use `blobs`; >= 0: frame index in the device blob bank       */
  int32_t it_since_init;     /* it_since_initialized_ (1 right after init, 2 steady state)      */
  int32_t force_iters;       /* 0: reference exit rule; > 0: run exactly this many iterations   */
  double dt;                 /* predicted_time_ - current_time_ (PE:499)                        */
  uint64_t seed;             /* replaces std::random_device (PE:476); reference mode uses low 32 */
  uint64_t frame_idx;        /* Philox counter word                                             */
} pfmpe_frame_in;

/* Per-frame outputs: the scalars the host needs after PE:733 */
typedef struct {
  int32_t iters;            /* PF iterations executed (k)                                        */
  int32_t kept_iter;        /* iteration whose particle set was kept (PE:608-624)                */
  int32_t most_likely_idx;  /* mostLikelyParticleIdx (PE:610; PE:714 on the re-init branch)      */
  int32_t accepted;         /* probPartSum != 0 && highestProb > M*min(3,B)  (PE:633)            */
  int32_t resampled;        /* stratified resampling ran (PE:666-682); new prior is resident     */
  int32_t winner_idx;       /* argmax resample count (PE:685-686), -1 if not resampled           */
  int32_t n_corr;           /* rows of correspondences_ for the winner (PE:688)                  */
  int32_t flag_fail;        /* PFMPE_FLAG_ACCEPTED / PFMPE_FLAG_REINIT                           */
  double highest_prob;      /* highestProb                                                        */
  double prob_sum;          /* probPartSum = sum of kept raw weights (PE:627)                     */
  double winner_pose[12];   /* PoseParticle[winner] -> predicted_pose_ before GN (PE:687);
                               on re-init: PoseParticle[most_likely_idx] (PE:716)                */
  double most_likely_pose[12]; /* PoseParticle[most_likely_idx]                                  */
  uint32_t corr[2 * PFMPE_MAX_MARKERS]; /* (LED, blob) 1-based pairs, extraction order (PE:2417) */
} pfmpe_frame_out;

/* ---------------------------------------------------------------------------------- lifetime */
/* Replaces the PoseEstimator member state of pose_estimator.h:65-70 (PoseParticle, newPoseEstimation,
 * probPart) with device-resident SoA buffers sized for max_particles. */
int pfmpe_create(pfmpe_ctx** out, int hip_device, int max_particles, int max_markers, int max_blobs,
                 int state_dtype);
void pfmpe_destroy(pfmpe_ctx* ctx);
const char* pfmpe_last_error(const pfmpe_ctx* ctx);
int pfmpe_abi_version(void);

/* ----------------------------------------------------------------------------------- model/params */
/* object_points_ (PoseEstimator::setMarkerPositions PE:56), camera_matrix_K_ (3x3 row-major,
 * monocular_pose_estimator.cpp:215-238) and bMarkerDowngrade (monocular_pose_estimator.cpp:510-517,
 * here one flag per marker; NULL = none). */
int pfmpe_set_model(pfmpe_ctx* ctx, const double* markers_xyz, int M, const double* K,
                    const uint8_t* downgrade);
/* Fills the PF parameter fields (dynamicParametersCallback, monocular_pose_estimator.cpp:480-527). */
int pfmpe_set_params(pfmpe_ctx* ctx, const pfmpe_params* params);
void pfmpe_default_params(pfmpe_params* params);

/* Sets N = N_Particle and the prior newPoseEstimation (N x 12).  Called after (re)initialisation,
 * which seeds the particle set (PE:1429-1437, 1756-1760). */
int pfmpe_set_prior(pfmpe_ctx* ctx, const double* poses, int N);

/* ------------------------------------------------------------------------------------- the step */
/* One PF step = PE:475-690 (+ PE:707-719): propagate, project, weigh (iterating per PE:535-616),
 * normalise, accept, stratified-resample, pick the winner.  Blocking. */
int pfmpe_step(pfmpe_ctx* ctx, const pfmpe_frame_in* in, pfmpe_frame_out* out);

/* n consecutive frames of one stream, in order, each exactly as pfmpe_step (blocking on its own frame
 * record before the next frame is launched) — the loop a C/C++ tracker runs, without per-call FFI
 * overhead.  Stops at the first error; *done receives the number of frames completed. */
int pfmpe_step_batch(pfmpe_ctx* ctx, const pfmpe_frame_in* in, int n, pfmpe_frame_out* out, int* done);

/* One frame of each of S independent contexts (camera streams / tracked objects: the reference's
 * per-object loop, PE:89, with per-object state PE:113-114, 726-727) as ONE batch on the device: the S
 * weighing passes run as one launch, the S resampling passes as a second, the S frame records as a third
 * (plus iteration batches for streams whose exit rule does not fire at once).  in[s] / out[s] belong to
 * ctxs[s]; each context's outputs and state equal what pfmpe_step(ctxs[s], &in[s], &out[s]) gives.
 * All contexts must be distinct, on one device, of one state type, RNG mode and pruning option; the batch
 * runs on ctxs[0]'s HIP stream and uses ctxs[0]'s batch scratch.  Work a member context has pending on
 * its own stream (an earlier pfmpe_step, ...) is ordered before the batch, and the member's next work on
 * its own stream after it (events, only when the streams differ).  Blocking.  At most
 * PFMPE_OPT_MULTI_MAX_BLOCKS (of ctxs[0]) 256-particle blocks per batch, in all: 160000 (~41M particles).
 * Errors (nothing launched): PFMPE_E_ARG for a mismatch, the failing stream's own pfmpe_step code
 * (E_ARG / E_CAP / E_STATE) for a bad frame, PFMPE_E_CAP above the block limit; the text, prefixed with
 * the stream index, in pfmpe_last_error(ctxs[0]).  With PFMPE_OPT_TIMING set on ctxs[0] the batch's
 * launches are timed into ctxs[0]'s kernel statistics (weighing, resampling, finishing, staging = aux). */
int pfmpe_step_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, pfmpe_frame_out* out);

/* n consecutive batches of pfmpe_step_multi (in / out: n x S, batch-major), each blocking on its records
 * before the next is launched — the loop a multi-object C/C++ tracker runs, without per-call FFI overhead.
 * Stops at the first error; *done receives the number of batches completed. */
int pfmpe_step_multi_batch(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, int n, pfmpe_frame_out* out,
                           int* done);

/* ---------------------------------------------------------------------- ROI prediction (§8f row 1) */
/* predictMarkerPositionsInImage (PE:1036-1053) + LEDDetector::determineROI (led_detector.cpp:217-369),
 * as called at PE:396-412: every marker projected through camMoveInv * prior_j * predictionMatrix for all
 * N particles of the current prior, plus the markers at predicted_pose_; the bounding box (x_min/y_min
 * from +inf, x_max/y_max from 0); its corners as cv::Point2f through distortPoints (plumb_bob D, in
 * double); border, clamp to the image, integer cv::Rect (the whole image when narrower than 1 px).
 * Call it before pfmpe_step of the same frame (the prior is the resampled set of the previous one).  The call is
 * pfmpe_predict_roi_multi (below) with S = 1: the same kernels and host path, on ctx's stream and scratch. */
typedef struct {
  double cam_move_inv[12];   /* camMoveInv (PE:241-393)                                          */
  double prediction[12];     /* predictionMatrix (PE:234)                                        */
  double predicted_pose[12]; /* predicted_pose_ (PE:1051)                                        */
  double D[5];               /* camera_distortion_coeffs_ k1 k2 p1 p2 k3 (led_detector.cpp:380)  */
  int32_t image_w, image_h;  /* image.size()                                                     */
  int32_t border;            /* roi_border_thickness_                                            */
  int32_t pad;
} pfmpe_roi_in;
typedef struct {
  int32_t x, y, width, height; /* region_of_interest_ (cv::Rect)                                 */
  double bbox[4];              /* undistorted x_min, x_max, y_min, y_max of the projections       */
} pfmpe_roi_out;
int pfmpe_predict_roi(pfmpe_ctx* ctx, const pfmpe_roi_in* in, pfmpe_roi_out* out);

#define PFMPE_ROI_MAX_STREAMS 64

/* The single call above for one frame of each of S contexts (the numUAV loop, PE:89, at PE:396-412) as one launch
 * sequence with one synchronise.  in[s] / out[s] belong to ctxs[s]; out[s] is what the single call on ctxs[s] with
 * in[s] returns: the same rectangle and the same bits of bbox.  Contexts: distinct, on one device, of one state
 * type; N, M, markers, K, the prior's storage (particle order or owner indices, fp16 anchor) and every field of
 * in[s] are per stream.  Runs on ctxs[0]'s stream and uses ctxs[0]'s scratch; work a member has pending elsewhere is
 * ordered before the batch; blocking, so nothing of the batch is pending when it returns.  Reads only: no context's
 * state changes.  With PFMPE_OPT_TIMING on ctxs[0] the sequence is one PFMPE_K_ROI bracket on ctxs[0] (DESIGN.md
 * §4.14: design and measured times).
 * Everything is checked before anything is staged or launched, and out is untouched on an error: PFMPE_E_ARG
 * (S < 1, NULL ctxs / in / out / ctxs[s], a context twice, a device or state-type mismatch, image_w / image_h < 1),
 * PFMPE_E_CAP (S > PFMPE_ROI_MAX_STREAMS), PFMPE_E_STATE (a stream without model or prior); the text,
 * "predict_roi_multi: stream <s>: ...", is the last-error text of ctxs[0]. */
int pfmpe_predict_roi_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_roi_in* in, pfmpe_roi_out* out);

/* host-only (no GPU, no context): the code a lane of the ROI kernels runs, for N caller-given poses (N x 12 doubles,
 * N >= 0; N = 0 leaves the markers at predicted_pose_ only), then the same host end (corner distortion, border,
 * clamp, cv::Rect).  For poses = the rows pfmpe_get_particles returns for the prior it equals the device calls, for
 * every state type.  PFMPE_E_ARG for a NULL pointer (poses may be NULL when N = 0), M outside 1..PFMPE_MAX_MARKERS,
 * N < 0, an image side < 1; out is untouched then. */
int pfmpe_host_predict_roi(const double* markers_xyz, int M, const double* K, const double* poses, int64_t N,
                           const pfmpe_roi_in* in, pfmpe_roi_out* out);

/* ------------------------------------------------- brute-force P3P (re)initialisation (§8f row 2) */
/* PoseEstimator::initialise (PE:1503-1786) for the particle-filter configuration, run when the track is
 * lost (it_since_initialized_ < 1, PE:128-205).  Blobs are image_points_ (undistorted px).  Stages:
 *   1. histogram (PE:1526-1716, device): for every 3-blob combination passing the spread filter
 *      (threshDist, >= 5 blobs near the centroid) x every ordered 3-marker permutation, P3P
 *      (p3p.cpp:65-292) gives 4 poses; each finite, non-repeated pose back-projects the unused markers
 *      through H.inverse() and, when at least one unused blob lies within tol of its nearest projection,
 *      the 3 P3P pairs and every such (blob, nearest marker) pair are counted;
 *   2. candidate correspondence vectors (correspondencesFromHistogram PE:1134-1288, host);
 *   3. checkCorrespondences of every candidate (PE:1312-1501; P3P over each 3-subset, device), the
 *      particle seeding and the fill loop (PE:1429-1437, 1755-1760), predicted_pose_ by
 *      computeTransformation (PE:2139-2161, host) for the first match.
 * tol = the context's params.tol (back_projection_pixel_tolerance_, shared with the PF score). */
typedef struct {
  double certainty_threshold;  /* certainty_threshold_ (PE:1411), README default 1                    */
  double valid_corr_threshold; /* valid_correspondence_threshold_ (PE:1477), README default 0.5        */
  int32_t n_particles;         /* N_Particle; 0 = the context's current N (max_particles if none)      */
  int32_t max_candidates;      /* cap on correspondence vectors (PFMPE_E_CAP beyond it); default 2^20  */
} pfmpe_init_params;
typedef struct {
  int32_t found;            /* initialise() == 1; the particle set is then seeded (see below)       */
  int32_t flag_fail;        /* 0 when found, else the last PubData.Flag_Fail code initialise wrote:
                               10 too few blobs, 12 empty histogram, 11 no candidate, 6 too few
                               correspondences, 9 P3P failed, 7 / 8 validity ratio; -1 none          */
  int32_t n_estimates;      /* P3P poses stored into PoseParticle (NumberOfP3PEstimation - 1)        */
  int32_t n_candidates;     /* correspondence vectors from the histogram                            */
  int32_t first_match;      /* candidate giving correspondences_ / predicted_pose_ (-1: none)      */
  int32_t n_corr;           /* rows of correspondences_                                             */
  uint32_t corr[2 * PFMPE_MAX_MARKERS]; /* (LED, blob) 1-based pairs                                 */
  double predicted_pose[12];/* predicted_pose_ (computeTransformation of the mean re-projections)   */
  uint64_t hist_total;      /* sum of the histogram                                                 */
} pfmpe_init_out;
void pfmpe_default_init_params(pfmpe_init_params* p);
/* Stage 1 alone: hist (B x M uint32, row-major: hist[blob * M + marker]).  3 <= B <= max_blobs (B < M included,
 * where pfmpe_initialise stops at flag 10): stage 1 of the batch below for one stream. */
int pfmpe_p3p_histogram(pfmpe_ctx* ctx, const double* blobs, int B, uint32_t* hist);
/* The whole initialise().  On success (out->found) the context's particle set becomes PoseParticle
 * (newPoseEstimation_Vec = PoseParticle, PE:191): slot N-k holds the k-th stored P3P pose (k = 1..K),
 * slots below repeat them with period K (the fill loop), and slot 0 keeps the resident set's slot 0
 * (identity if there is none) unless K >= N.  hist (optional, B x M) receives stage 1's histogram.  The call is
 * pfmpe_initialise_multi (below) with S = 1: the same kernels and host stages, on ctx's stream and scratch. */
int pfmpe_initialise(pfmpe_ctx* ctx, const double* blobs, int B, const pfmpe_init_params* params,
                     pfmpe_init_out* out, uint32_t* hist);

#define PFMPE_INIT_MAX_STREAMS 64

/* The single call above for S contexts as one batch (the numUAV loop, PE:89, in the branch it_since_initialized_ < 1,
 * PE:128-205: every object on the first frame, any number of them after a shared occlusion): one upload, one launch
 * sequence and one synchronise per stage, three synchronises per batch where S single calls make 3 x S.  in[s],
 * params[s] (params = NULL: the defaults for all), out[s] and hist[s] (hist = NULL or hist[s] = NULL: not wanted, else
 * B_s x M_s) belong to ctxs[s].  out[s], hist[s] and the particle set of ctxs[s] afterwards are what
 * pfmpe_initialise(ctxs[s], in[s].blobs, in[s].B, &params[s], &out[s], hist[s]) gives: out[s] byte for byte
 * (predicted_pose included), the histogram entry for entry, the seeded prior the same bits from
 * pfmpe_get_particles(ctxs[s], 1, ...): the single call is the batch of one, the counts are order-free integer sums
 * of per-item decisions, and the host stages run per stream.  Per stream: M, the markers, K and params.tol (from the context), B,
 * every field of params[s], and N by the single call's rule.  Contexts of any state types may be mixed (the device
 * stages are fp64, only the final import is typed); they must be distinct and on one device.  ctxs[0] leads: the
 * batch runs on its stream and in its initialisation scratch (grown once per stage to the batch's size), fills its
 * last-error text, and with PFMPE_OPT_TIMING on ctxs[0] is one PFMPE_K_P3P_HIST bracket and one PFMPE_K_P3P_CHECK
 * bracket of ctxs[0] (nothing is added to another context's statistics).  Work a member has pending on its own stream
 * is ordered before the batch; blocking, so nothing of the batch is pending when it returns.  A stream that is not
 * found (B < M: flag 10; an empty histogram: 12; no candidate: 11 / 6 / 7 / 8 / 9) keeps its particle set untouched
 * and does not affect the other streams; hist[s] is not written for a stream with B < M.
 * Everything is checked before anything is staged or launched; on such an error out and hist are untouched and no
 * context's state changes: PFMPE_E_ARG (S < 1, NULL ctxs / in / out / ctxs[s], a context twice, a device mismatch,
 * B < 0, NULL blobs with B > 0, M < 3), PFMPE_E_CAP (S > PFMPE_INIT_MAX_STREAMS, a stream's B > max_blobs,
 * n_particles > max_particles), PFMPE_E_STATE (a stream without a model); the text, "initialise_multi: stream <s>:
 * ...", is the last-error text of ctxs[0].  With ctxs = NULL or ctxs[0] = NULL: PFMPE_E_ARG, no text.
 * A candidate explosion is a run-time result, found after stage 1: when the correspondence vectors of stream s exceed
 * its max_candidates the call returns PFMPE_E_CAP with the same "stream <s>: " prefix.  By then the histograms of
 * stage 1 have been written to hist (every stream with B >= M); out is untouched and no context is seeded. */
typedef struct {
  const double* blobs;   /* B x 2 undistorted px (image_points_), host pointer; may be NULL when B == 0 */
  int32_t B;
  int32_t pad;
} pfmpe_init_in;         /* 16 bytes */
int pfmpe_initialise_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_init_in* in, const pfmpe_init_params* params,
                           pfmpe_init_out* out, uint32_t* const* hist);

/* host-only (no GPU, no context): the work mapping of the batch's histogram stage, which the call above launches
 * exactly.  Streams are grouped by the unused-marker bucket of their M (one launch per bucket present).  A stream
 * wants ceil(items / 256) blocks of 256 threads; a bucket's launch holds at most 8 * max(num_cu, 1) blocks;
 * when the wants of a bucket exceed it, stream s gets floor(want_s * cap / wants) blocks, and one block
 * where that is zero, so the launch exceeds the cap by at most one block per stream with work.  Block b (counted from
 * first_block) of a stream with `blocks` blocks visits the items b * 256 + t + k * blocks * 256 (thread t, round k).
 * blocks_per_bucket: the three launches' sizes (0: no launch).  PFMPE_E_ARG for a NULL pointer, S outside
 * 1..PFMPE_INIT_MAX_STREAMS, M outside 3..PFMPE_MAX_MARKERS or B < 0, PFMPE_E_CAP for B > PFMPE_MAX_BLOBS; the
 * outputs are untouched then. */
typedef struct {
  int64_t items;        /* C(B,3) * M(M-1)(M-2); 0 when B < M or B < 3                                   */
  int32_t first_block;  /* first block of this stream in its launch                                      */
  int32_t blocks;       /* blocks given to it (0 when items == 0)                                        */
  int32_t bucket;       /* 0 / 1 / 2: the unused-marker bucket (M - 3 <= 2, <= 9, else)                  */
  int32_t lds_hist;     /* 1: histogram in LDS (B * M * 4 <= 32 KiB), 0: global atomics                  */
} pfmpe_init_plan;      /* 24 bytes */
int pfmpe_host_init_plan(const int32_t* M, const int32_t* B, int S, int num_cu, pfmpe_init_plan* plan,
                         int32_t* blocks_per_bucket);

/* ---------------------------------------------------------------- LED detector (§8f row 4) */
/* LEDDetector::findLeds (pf_mpe_lib/src/led_detector.cpp:46-215) on the device for one ROI of an 8-bit
 * grey image: threshold (THRESH_TOZERO for active markers, else THRESH_BINARY_INV), GaussianBlur (ksize
 * from sigma, OpenCV 2.4's 8-bit integer separable path, reflect-101), findContours(RETR_EXTERNAL,
 * CHAIN_APPROX_NONE) with 2.4's zeroed 1-pixel frame, contourArea / boundingRect / moments, the blob
 * size-aspect-circularity filter, the centre + ROI offset (cv::Point2f) and undistortPoints(K, D, P = K).
 * K is the context's model K.  Output: image_points_ (undistorted px, findContours order) and the
 * distorted centres (distorted_detection_centers_).  image = NULL uses the staged image.  blobs: max_out x 2
 * doubles, distorted: max_out x 2 floats (may be NULL); min(n, max_out, PFMPE_MAX_BLOBS) rows are written and
 * nothing else of the arrays is touched. */
typedef struct {
  int32_t threshold_value;          /* detection_threshold_value_ (threshold_value, README default 240) */
  int32_t active_markers;           /* 1: THRESH_TOZERO, 0: THRESH_BINARY_INV (LD:56-59)               */
  double gaussian_sigma;            /* gaussian_sigma_ (0.6), in (0, 5]                               */
  double min_blob_area;             /* min_blob_area_ (the tracker's adapted value, PE:432-435)       */
  double max_blob_area;             /* max_blob_area_                                                 */
  double max_width_height_distortion; /* 0.7                                                          */
  double max_circular_distortion;   /* 0.7                                                            */
  double D[5];                      /* camera_distortion_coeffs_ k1 k2 p1 p2 k3                       */
  int32_t roi_x, roi_y, roi_w, roi_h; /* region_of_interest_; roi_w / roi_h < 0 = the whole image   */
} pfmpe_detect_params;
typedef struct {
  int32_t n;                        /* detections (all of them; min(n, max_out, PFMPE_MAX_BLOBS) written) */
  int32_t n_components;             /* 8-connected components (contours) found, all of them           */
  int32_t overflow;                 /* more than 8192 components: 8192 of them were examined (which   */
                                    /* ones is unspecified); n counts the detections among those      */
  int32_t pad;
} pfmpe_detect_out;
void pfmpe_default_detect_params(pfmpe_detect_params* p);
int pfmpe_stage_image(pfmpe_ctx* ctx, const uint8_t* image, int width, int height, int pitch);
int pfmpe_find_leds(pfmpe_ctx* ctx, const uint8_t* image, int width, int height, int pitch,
                    const pfmpe_detect_params* params, double* blobs, float* distorted, int max_out,
                    pfmpe_detect_out* out);

#define PFMPE_DETECT_MAX_ROIS 64

/* R ROIs of one image, one launch sequence, one synchronise: the per-object findLeds calls of a multi-object
 * tracker (the numUAV loop, PE:89, PE:442) and their retries on an enlarged ROI (PE:452-463) as one batch.
 * params[r] is a complete pfmpe_detect_params with its own ROI, threshold, sigma, area limits, D, active_markers;
 * ROIs may overlap, repeat, or be the whole image (roi_w / roi_h < 0).  blobs: R x max_out x 2 doubles,
 * distorted: R x max_out x 2 floats (may be NULL), ROI r at offset r * 2 * max_out; out: R records.
 * image = NULL uses the staged image.  ROI r's rows and out[r] are what the single-ROI call returns for params[r]
 * (same detections, same order, same bits, while overflow is 0): out[r].n counts all detections,
 * min(n, max_out, PFMPE_MAX_BLOBS) rows are written and nothing else of the arrays is touched.  Everything is
 * checked before anything is staged or launched and out is untouched on an error: PFMPE_E_ARG (R < 1, a NULL
 * pointer, max_out < 0, an ROI outside the image or gaussian_sigma outside (0, 5]: the error text names the
 * entry, "find_leds_multi: roi <r>: ..."), PFMPE_E_CAP (R > PFMPE_DETECT_MAX_ROIS), PFMPE_E_STATE (no model, or
 * image = NULL without a staged image of that size).  Blocking, on the context's stream; with PFMPE_OPT_TIMING
 * the sequence is one PFMPE_K_DETECT bracket. */
int pfmpe_find_leds_multi(pfmpe_ctx* ctx, const uint8_t* image, int width, int height, int pitch,
                          const pfmpe_detect_params* params, int R, double* blobs, float* distorted,
                          int max_out, pfmpe_detect_out* out);

#define PFMPE_DETECT_MAX_IMAGES 64

/* R detector entries over the images of up to PFMPE_DETECT_MAX_IMAGES cameras, one launch sequence, one
 * synchronise: the detector stage of a multi-camera frame, between the batched ROI prediction and the batched PF
 * step.  Entry r detects in images[image_of[r]] with params[r] (a complete record, as for the one-image batch) and
 * with K of that image's context; blobs / distorted / out are laid out as for the one-image batch (R x max_out x 2,
 * out[r]).  Entry r's rows and out[r] are the bits the single-ROI call on images[image_of[r]].ctx returns for that
 * image and params[r] while overflow is 0; min(n, max_out, PFMPE_MAX_BLOBS) rows are written and nothing else of the
 * arrays is touched.  Of a host image only the pixels of its entries' ROIs cross the host link (the upload plan
 * below); image = NULL reads the context's staged image in place.  Contexts of any state types may be mixed and a
 * context may appear under several images; all must be on one device.  images[0].ctx leads: the batch runs on its
 * stream, in its batch scratch, fills its last-error text and is one PFMPE_K_DETECT bracket of its timing (nothing
 * is added to another context's statistics).  Blocking.  No context's staged image, model or particle state changes.
 * Everything is checked before anything is packed, staged or launched and out is untouched on an error:
 * PFMPE_E_ARG (a NULL pointer or a NULL ctx; I < 1, R < 1, max_out < 0, an image_of[r] outside 0 .. I - 1; an image
 * with width or height < 1 or pitch < width; contexts on different devices; an ROI outside its image or
 * gaussian_sigma outside (0, 5]: "find_leds_streams: roi <r>: ..."), PFMPE_E_CAP (R > PFMPE_DETECT_MAX_ROIS or
 * I > PFMPE_DETECT_MAX_IMAGES), PFMPE_E_STATE (a context without a model, or image = NULL on a context with no staged
 * image of that width, height and pitch).  With images = NULL or images[0].ctx = NULL: PFMPE_E_ARG, no error text. */
typedef struct {
  pfmpe_ctx* ctx;        /* the camera's context: K of its model; its staged image when image == NULL   */
  const uint8_t* image;  /* host, 8-bit grey; NULL = ctx's staged image                                 */
  int32_t width, height, pitch, pad;
} pfmpe_detect_image;    /* 32 bytes */
int pfmpe_find_leds_streams(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                            const pfmpe_detect_params* params, int R, double* blobs, float* distorted, int max_out,
                            pfmpe_detect_out* out);

/* host-only (no GPU, no context: the ctx fields may be NULL): the upload plan of the call above, and its pack.
 * An entry's rectangle is its ROI in its image (roi_w < 0: the whole width, roi_h < 0: the whole height).  An entry
 * on a staged image gets offset -1, the image's pitch and shared_with -1.  An entry r on a host image is served by
 * its owner: of the entries of the same image index whose rectangle contains r's (r included), the one of the
 * largest area, the lowest index on a tie.  An entry that owns itself has its own crop: pitch = its width rounded
 * up to a multiple of 16, start 256-byte aligned, own crops in ascending entry index with no other gaps.  An entry
 * owned by q has shared_with = q, q's pitch and offset = crops[q].offset + (y_r - y_q) * pitch + (x_r - x_q): the
 * retry on an enlarged ROI (PE:452-463) uploads nothing extra.  upload_bytes: the end of the last own crop rounded
 * up to 256 (0 without an own crop).  The pack copies every own crop's rows out of the caller's images (pageable,
 * any pitch >= width) to the planned offsets and writes every other byte of buffer[0 .. upload_bytes) as 0; crops
 * must be the plan of the same batch.  Errors leave the outputs untouched: the geometric checks and codes of the
 * call above, PFMPE_E_ARG for crops that are not the batch's plan, PFMPE_E_CAP for buffer_bytes < upload_bytes. */
typedef struct {
  int64_t offset;        /* byte offset of the entry's top-left ROI pixel in the upload buffer; -1: staged image */
  int32_t pitch;         /* row pitch at that offset                                                    */
  int32_t shared_with;   /* -1: own crop (or staged); else the entry whose crop holds this entry's pixels */
} pfmpe_detect_crop;     /* 16 bytes */
int pfmpe_host_detect_plan(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                           const pfmpe_detect_params* params, int R, pfmpe_detect_crop* crops,
                           int64_t* upload_bytes);
int pfmpe_host_detect_pack(const pfmpe_detect_image* images, int I, const int32_t* image_of,
                           const pfmpe_detect_params* params, int R, const pfmpe_detect_crop* crops,
                           uint8_t* buffer, int64_t buffer_bytes);

/* host-only: the reference's ROI enlargement (PE:429-432 with margin = ROI_distVal, PE:454-457 with margin = 20):
 *   x' = max(x - margin, 0), y' = max(y - margin, 0),
 *   w' = min(w + 2 margin, image_w - x'), h' = min(h + 2 margin, image_h - y')   (note: x', y', as the reference)
 * roi / grown: x, y, w, h.  PFMPE_E_ARG for a NULL pointer, margin < 0 or an image side < 1. */
int pfmpe_host_grow_roi(const int32_t roi[4], int32_t margin, int32_t image_w, int32_t image_h, int32_t grown[4]);

/* ---------------------------------------- configuration files and recorded streams (§8f row 3) */
/* Host-only (no GPU): pfmpe_io.cpp.  The reference reads these through ROS (rosparam / getParam /
 * dynamic_reconfigure, pf_mpe/src/monocular_pose_estimator.cpp:81-126, 479-527) and the CameraInfo topic.
 * Marker YAML (README.md:95-117): `marker_positions:` followed by a list of {x, y, z} maps (block or flow
 * style).  Writes min(count, max_markers) rows of xyz; returns the number of markers, or < 0. */
int pfmpe_parse_marker_yaml(const char* text, double* xyz, int max_markers);
/* The PF / initialisation / marker-split parameters of a ROS launch file (<param name=.. value=../>,
 * pf_mpe/launch/<name>.launch): the names dynamicParametersCallback copies into PoseEstimator.  Absent names
 * keep the defaults of pfmpe_default_launch_config (the engine's defaults).  Returns how many names
 * were recognised. */
typedef struct {
  pfmpe_params pf;                       /* back_projection_pixel_tolerance(_PF), min/maxAngularNoise,
                                            min/maxTransitionNoise                                       */
  pfmpe_init_params init;                /* certainty_threshold, valid_correspondence_threshold, N_Particle */
  int32_t num_objects;                   /* numUAV                                                       */
  int32_t markers_per_object[4];         /* numberOfMarkersUAV1..4: split of the marker list per object  */
  int32_t use_particle_filter;           /* bUseParticleFilter                                           */
  uint8_t downgrade[PFMPE_MAX_MARKERS];  /* bMarkerNr1..5 -> bMarkerDowngrade                           */
} pfmpe_launch_config;
void pfmpe_default_launch_config(pfmpe_launch_config* cfg);
int pfmpe_parse_launch(const char* text, pfmpe_launch_config* cfg);
/* sensor_msgs/CameraInfo as echoed in README.md:127-143: K (9, row-major), D (plumb_bob k1 k2 p1 p2 k3),
 * width, height (any pointer may be NULL).  Returns a bit mask of what was found (1 K, 2 D, 4 width,
 * 8 height) or < 0 on a malformed K / D list. */
int pfmpe_parse_camera_info(const char* text, double* K, double* D, int32_t* width, int32_t* height);
/* Recorded detection streams (image_points_ per frame, undistorted px), little-endian binary:
 *   header "PFMB" | u32 version = 1 | u32 n_frames | u32 reserved
 *   frame  f64 timestamp | u32 B | u32 flags = 0 | B x {f64 x, f64 y}
 * offsets: n_frames + 1 prefix offsets into blobs (rows), as pfmpe_stage_blob_bank.  read: call with
 * NULL buffers to get n_frames / n_blobs; PFMPE_E_CAP if the buffers are too small. */
int pfmpe_write_blob_stream(const char* path, const double* timestamps, const double* blobs, const int32_t* offsets,
                            int n_frames);
int pfmpe_read_blob_stream(const char* path, double* timestamps, double* blobs, int32_t* offsets, int max_frames,
                           int64_t max_blobs, int* n_frames, int64_t* n_blobs);
/* Reads a stream file and stages every frame in the context's device blob bank (bank_frame = index). */
int pfmpe_stage_blob_stream(pfmpe_ctx* ctx, const char* path, int* n_frames);

/* getPoseParticles (PE:917, which = 0: kept propagated set of the last step) and getResampledParticles
 * (PE:923, which = 1: current prior).  N x 12 doubles. */
int pfmpe_get_particles(pfmpe_ctx* ctx, int which, double* out);
/* probPart of the last step: the kept iteration's raw (un-normalised) weights, N doubles. */
int pfmpe_get_weights(pfmpe_ctx* ctx, double* out);
/* counterMeas of the last step (PE:524, 678): N uint32; requires PFMPE_OPT_RECORD_COUNTS. */
int pfmpe_get_counts(pfmpe_ctx* ctx, uint32_t* out);

/* ------------------------------------------------------------- statistics of the particle cloud */
/* Posterior mean, 6x6 covariance and effective sample size of a particle set, reduced on the device (the
 * particles stay in HBM; 60 doubles come back).  The covariance is in the coordinates of the reference's
 * pose_covariance_ (A.inverse() of the Gauss-Newton step, PE:2004, getPoseCovariance): twists [upsilon; omega]
 * (translation part first, exponentialMap / logarithmMap PE:2194-2296) of a left perturbation of a reference
 * pose, T = exp(xi) * T_ref, as in T_new = exponentialMap(dT) * predicted_pose_ (PE:1876).
 *
 * Definition.  For particle pose T_i = [R_i | t_i] and the caller's T_ref = [R_r | t_r]:
 *   D = T_i * T_ref^-1 with T_ref^-1 = [R_r^T | -R_r^T t_r]:  D_R = R_i R_r^T,  d = t_i - D_R t_r
 *   a = 1/2 (D_R[2,1] - D_R[1,2], D_R[0,2] - D_R[2,0], D_R[1,0] - D_R[0,1]),  s = |a|,  c = 1/2 (tr D_R - 1)
 *   phi = atan2(s, c);  omega = f a,  f = phi / s when s > 1e-8, else 1 + s^2 / 6
 *   upsilon = (I - 1/2 omega^ + k omega^ omega^) d,
 *     k = (1 - phi sin phi / (2 (1 - cos phi))) / phi^2 when phi >= 1e-4, else 1/12 + phi^2 / 720
 *     (1 - cos phi is evaluated as 2 sin^2(phi / 2))
 *   xi_i = [upsilon; omega];  a pose bit-equal to T_ref has xi_i = 0 exactly.
 * The formula is applied to the stored matrices as they are: fp32 / fp16 state is only approximately
 * orthonormal and is not re-orthonormalised.  Clouds near phi = pi are out of scope (omega is ill-defined there).
 * With weights w_i >= 0:
 *   W = sum w,  mu = sum w xi / W,  C = sum w xi xi^T / W - mu mu^T (symmetric, row-major, both triangles),
 *   ESS = W^2 / sum w^2,  mean_pose = exp(mu) * T_ref (exp as PE:2194-2226),
 *   max_trans = max |upsilon_i|, max_rot = max |omega_i| over particles with w_i > 0 (the cloud's extent).
 * mean_pose is ONE step toward the intrinsic mean: a caller who wants to iterate calls again with mean_pose
 * as the reference.  All arithmetic is fp64 for every state type; the sums have a fixed order that depends on
 * N alone, so a repeated call returns the same bits.
 *
 * Blocking; runs on the context's stream (after the last frame, before the next).  Changes nothing the next
 * frame reads.  Not timed by PFMPE_OPT_TIMING (there is no kernel-statistics slot for it; regenerating the
 * WEIGHTED set counts as aux, as for the particle read-back).  The call is pfmpe_cloud_stats_multi (below) with one
 * entry: the same kernels and host path, on ctx's stream and scratch.
 * Errors: PFMPE_E_ARG for a bad `which`, a NULL pointer or a non-finite reference pose; PFMPE_E_STATE with no
 * particle set, and for WEIGHTED before the first step. */
enum { PFMPE_CLOUD_WEIGHTED = 0,   /* kept propagated set of the last step with probPart as weights
                                      (the rows of pfmpe_get_particles(0) and pfmpe_get_weights)            */
       PFMPE_CLOUD_POSTERIOR = 1 };/* current prior = resampled set, unit weights (pfmpe_get_particles(1)) */
typedef struct {
  int64_t n;               /* particles reduced                                  */
  int32_t degenerate;      /* 1: W == 0 (all weights zero); means / cov are 0 and mean_pose = ref */
  int32_t pad;
  double wsum, ess;        /* W, ESS (0 when degenerate)                         */
  double mean_twist[6];    /* mu                                                 */
  double cov[36];          /* C                                                  */
  double mean_pose[12];
  double max_trans, max_rot;
} pfmpe_cloud_out;
int pfmpe_cloud_stats(pfmpe_ctx* ctx, int which, const double* ref_pose12, pfmpe_cloud_out* out);

#define PFMPE_CLOUD_MAX_STREAMS 64

/* The single call above for S entries (the statistics of every object of a frame, pose_covariance_Vec[objectNumber]
 * of the numUAV loop, PE:89) as one launch sequence with one synchronise.  out[s] is byte for byte what
 * pfmpe_cloud_stats(ctxs[s], in[s].which, in[s].ref_pose, &out[s]) writes, the degenerate record of an entry whose
 * weights are all zero included.  `which` and the reference pose are per entry; N, the prior's storage (particle
 * order or owner indices, fp16 anchor) and the kept iteration are the context's.  A context may appear in several
 * entries (both sets of one object, or two reference poses); a context with at least one WEIGHTED entry regenerates
 * its kept propagated set once, and all its entries read that set.  Contexts: on one device, of one state type.
 * Runs on ctxs[0]'s stream and uses scratch ctxs[0] owns; work a member has pending elsewhere (its regeneration, on
 * its own stream, included) is ordered before the batch; blocking.  Reads only: no context's state changes.  Not timed
 * by PFMPE_OPT_TIMING, as the single call is not (a member's regeneration counts as aux on that member).  DESIGN.md
 * §4.11a: design and measured times.
 * Everything is checked before anything is staged, regenerated or launched, and out is untouched on an error:
 * PFMPE_E_ARG (S < 1, NULL ctxs / in / out / ctxs[s], a device or state-type mismatch, a bad `which`, a non-finite
 * reference pose), PFMPE_E_CAP (S > PFMPE_CLOUD_MAX_STREAMS), PFMPE_E_STATE (an entry whose context has no particle
 * set, or a WEIGHTED entry before that context's first step); the text, "cloud_stats_multi: stream <s>: ...", is the
 * last-error text of ctxs[0].  With ctxs == NULL or ctxs[0] == NULL: PFMPE_E_ARG and no text. */
typedef struct {
  double ref_pose[12];   /* T_ref of this entry */
  int32_t which;         /* PFMPE_CLOUD_WEIGHTED / PFMPE_CLOUD_POSTERIOR */
  int32_t pad;
} pfmpe_cloud_in;        /* 104 bytes */
int pfmpe_cloud_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_cloud_in* in, pfmpe_cloud_out* out);

/* host-only (no GPU, no context): the grid a pfmpe_cloud_stats_multi batch launches for entries of N[s] particles.
 * Entry s gets blocks = min(ceil(N[s] / 256), 1024), the single call's grid, so its sums have the single call's
 * order; first_block is the running sum of blocks and *total_blocks the flat grid's size.  PFMPE_E_ARG for a NULL
 * pointer, S < 1 or an N < 1; PFMPE_E_CAP for S > PFMPE_CLOUD_MAX_STREAMS; the outputs are untouched then. */
typedef struct { int32_t first_block, blocks; } pfmpe_cloud_plan;   /* 8 bytes */
int pfmpe_host_cloud_plan(const int32_t* N, int S, pfmpe_cloud_plan* plan, int32_t* total_blocks);

/* The cloud's mass and statistics per hypothesis.  pfmpe_top_particles names the K best distinct hypotheses of a frame
 * (the winner and the mirror solution of a near-symmetric LED set); pfmpe_cloud_stats describes the whole cloud with
 * one mean and one covariance, which between two modes describe neither.  pfmpe_cloud_modes assigns every particle to
 * the nearest of K seed poses (from pfmpe_top_particles, or the caller's) and returns the record of pfmpe_cloud_stats
 * per mode: how much of the posterior sits in each hypothesis, and how wide each one is.  No per-particle array moves
 * to the host unless the caller asks for mode_of.
 *
 * Set: `which` as for pfmpe_cloud_stats: WEIGHTED the rows of pfmpe_get_particles(0) with pfmpe_get_weights,
 * POSTERIOR the rows of pfmpe_get_particles(1) with unit weights.
 * Distance of particle pose p to seed s, in fp64 on the 12-double rows, every product and sum rounded on its own, left
 * to right, with d2 and tr exactly those of pfmpe_top_particles' predicate for the pair (p, s):
 *   d2 = (tp0-ts0)^2 + (tp1-ts1)^2 + (tp2-ts2)^2;   tr = sum of Rp[r][c]*Rs[r][c] over the nine entries, row-major
 *   a = d2 * it2,  b = (3.0 - tr) * ir2,  dist = a + b
 *   it2 = trans_scale > 0 ? 1 / (trans_scale * trans_scale) : 0, ir2 likewise from rot_scale (formed once on the host)
 * 3 - tr is 2 (1 - cos theta) ~ theta^2 of the relative rotation; rounding may leave it slightly negative, which is
 * allowed.  A scale of 0 takes its part out of the distance.
 * Assignment: best = +inf, mode = PFMPE_MODE_NONE; for k = 0 .. K-1: if (dist_k < best) { best = dist_k; mode = k; },
 * so the lowest k wins a tie; a NaN or infinite dist_k (of either sign) never wins.  With max_dist > 0 a particle with
 * !(best <= max_dist) becomes PFMPE_MODE_NONE.
 * Records: out[k].stats is the record pfmpe_cloud_stats defines, taken over the members of mode k alone with
 * T_ref = seeds[k]: every sum runs in the order pfmpe_cloud_stats uses for this N with the non-members skipped, n is the
 * member count, and a mode without weight (no members, or members of weight 0) has the degenerate record.  out[K] is the
 * same record of the PFMPE_MODE_NONE particles about seeds[0]; its mean_pose is where a caller would put the next
 * seed.  share = stats.wsum / (out[0].stats.wsum + ... + out[K].stats.wsum, added in index order), 0 if that sum is
 * 0.  mode_of, when given, receives every particle's mode (N bytes).
 * Hence: with K = 1, max_dist = 0 and finite poses, out[0].stats is byte for byte what
 * pfmpe_cloud_stats(ctx, which, seeds, .) writes, share is 1 and out[1] is the degenerate record with n = 0; a
 * repeated call returns the same bytes; moving another seed without changing any particle's mode leaves a mode's
 * record unchanged; the member counts sum to N; for POSTERIOR stats.wsum == stats.n exactly.
 *
 * Blocking; runs on the context's stream; reads only.  Not timed by PFMPE_OPT_TIMING (regenerating the WEIGHTED set
 * counts as aux).  The records come from the kernels and the host path of pfmpe_cloud_stats_multi: one batch of K + 1
 * entries on this context, each restricted to its mode.  DESIGN.md §4.16.
 * Errors, all checked before anything is staged or launched (out and mode_of stay untouched): PFMPE_E_ARG for a NULL
 * ctx, seeds or out, a bad `which`, K outside 1..PFMPE_MODES_MAX, a non-finite seed, a negative, NaN or infinite scale
 * or max_dist, both scales 0; PFMPE_E_STATE as pfmpe_cloud_stats.  The text begins "cloud_modes: ". */
#define PFMPE_MODES_MAX 16     /* largest K */
#define PFMPE_MODE_NONE 255    /* mode_of value of a particle no seed takes */
typedef struct {
  double trans_scale;  /* m,   >= 0, finite; 0: translation does not count            */
  double rot_scale;    /* rad, >= 0, finite; 0: rotation does not count (not both 0)   */
  double max_dist;     /* >= 0, finite; 0: no gate                                     */
} pfmpe_modes_params;  /* 24 bytes */
typedef struct {
  pfmpe_cloud_out stats;  /* of the mode's members about its seed; stats.n = members   */
  double share;           /* stats.wsum / (sum of all K + 1 wsum, in index order); 0 if that sum is 0 */
} pfmpe_mode_out;         /* 488 bytes */
void pfmpe_default_modes_params(pfmpe_modes_params* p);   /* 0.01, 0.05, 0 */
int pfmpe_cloud_modes(pfmpe_ctx* ctx, int which, const double* seeds /* K x 12 */, int K,
                      const pfmpe_modes_params* params /* NULL: defaults */,
                      pfmpe_mode_out* out /* K + 1 */, uint8_t* mode_of /* N bytes, may be NULL */);
/* host-only (no GPU, no context): the assignment alone, for N caller-given poses (N x 12), by the function the device
 * runs.  mode_of: N bytes; counts, when given: the members of modes 0 .. K-1, then the PFMPE_MODE_NONE particles
 * (they sum to N).  A non-finite pose is not an error: it has no mode.  PFMPE_E_ARG for the argument errors above,
 * N < 0, a NULL mode_of or NULL poses with N > 0; the outputs are untouched then. */
int pfmpe_host_cloud_assign(const double* poses, int64_t N, const double* seeds, int K,
                            const pfmpe_modes_params* params, uint8_t* mode_of, int64_t* counts /* K + 1, may be NULL */);

/* A new prior of n_new particles from the members of the current one, on the device: change the particle count of a
 * context (a wide cloud for acquisition, a small one for steady tracking: a frame of up to 131k particles is one
 * launch), keep one hypothesis and drop the others, or hand one hypothesis to a second context.  A lossless gather of
 * stored state: no pose crosses the host link and none is converted.
 *
 * Source set: src's current prior, the N rows pfmpe_get_particles(src, 1) returns (the posterior, unit weights).
 * Members: with K = 0 every particle; with K > 0 the particles n with mode_of[n] == mode, mode_of being what
 * pfmpe_cloud_modes(src, PFMPE_CLOUD_POSTERIOR, seeds, K, &modes, ., mode_of) writes (the same function assigns them).
 * Rank: let m be the member count and j_0 < j_1 < ... < j_(m-1) the members in ascending particle index.  New particle
 * k, 0 <= k < n_new, is a copy of source particle j_r with r = ((2k + 1) * m) / (2 * n_new) in unsigned 64-bit integers
 * (no overflow: 2k + 1 < 2^32, m < 2^31).  This is systematic resampling of unit weights with offset 1/2 and no random
 * draw: r is non-decreasing in k, every member is used floor or ceil of n_new / m times when n_new >= m, the ranks are
 * distinct and floor or ceil of m / n_new apart when n_new < m, and n_new == m is the identity on the members.  The
 * prior is sorted by owner (stratified resampling writes ascending owners), so equal-spaced picks of it are a systematic
 * resample of the same distribution: the posterior stays a posterior.
 * Copy: the 12 state elements of the source row as stored (fp64, fp32, or the fp16 deltas; a deferred prior is read
 * through its owner indices), and for fp16 state dst takes the anchor of src's set.  Hence for every state type, bit
 * for bit, pfmpe_get_particles(dst, 1)[k] after the call == pfmpe_get_particles(src, 1)[source[k]] before it, with
 * source from pfmpe_host_resample_source for the same mode_of; a repeated call gives the same bytes.
 *
 * Contexts: dst == src resamples in place; dst != src fills another context (a fork) and leaves src untouched.  Both
 * must be on one device and of one state type; max_particles, model and parameters may differ, and dst needs neither a
 * model nor a prior of its own.  The new prior goes to the state buffer dst's prior does not occupy, in particle order,
 * and becomes the prior only once the device work has been waited for: a failure leaves dst as it was.  Afterwards dst
 * is as after pfmpe_set_prior: N = n_new, no kept set of an earlier step (PROPAGATED / WEIGHTED calls and
 * pfmpe_get_counts return PFMPE_E_STATE until the next step), hand-off state zeroed.  The set is a posterior, not a
 * fresh initialisation: the caller keeps passing its own it_since_init.
 * No members (n_members == 0) is an outcome, not an error: PFMPE_OK, out->n_new = 0 and dst unchanged, its kept set
 * included.
 * Blocking; runs on dst's stream, after whatever src has pending on another stream.  Not timed by PFMPE_OPT_TIMING.
 * The scratch (a byte and 4/256 B per source particle, with a filter only) is dst's, grown on demand.  DESIGN.md §4.18.
 * Errors, all checked before anything is launched (out untouched, no context changed; the text, in dst's last error,
 * begins "resample_prior: "): PFMPE_E_ARG for a NULL dst (no text), src, params or out, n_new < 1, a device or
 * state-type mismatch, K outside 0..PFMPE_MODES_MAX, and with K > 0 NULL or non-finite seeds, the scale and max_dist
 * errors of pfmpe_cloud_modes, a mode that is neither 0..K-1 nor PFMPE_MODE_NONE; PFMPE_E_CAP for n_new above dst's
 * max_particles; PFMPE_E_STATE for a src without a particle set. */
typedef struct {
  int32_t n_new;             /* particles of the new prior, 1 .. dst's max_particles                          */
  int32_t K;                 /* 0: every particle is a member; 1..PFMPE_MODES_MAX: seeds, as pfmpe_cloud_modes */
  const double* seeds;       /* K x 12; may be NULL when K == 0                                                */
  int32_t mode;              /* K > 0: the mode kept, 0..K-1 or PFMPE_MODE_NONE; ignored when K == 0           */
  int32_t pad;
  pfmpe_modes_params modes;  /* K > 0: scales and gate, pfmpe_cloud_modes' rules; ignored when K == 0          */
} pfmpe_resample_params;     /* 48 bytes */
typedef struct {
  int64_t n_src;      /* particles of src's prior                                            */
  int64_t n_members;  /* of them, members                                                    */
  int64_t n_new;      /* particles of dst's new prior; 0 when n_members == 0 (dst unchanged) */
} pfmpe_resample_out;        /* 24 bytes */
int pfmpe_resample_prior(pfmpe_ctx* dst, pfmpe_ctx* src, const pfmpe_resample_params* params,
                         pfmpe_resample_out* out);
/* host-only (no GPU, no context): the source particle of every new slot by the rule above, for the members
 * mode_of[n] == mode of N particles (mode_of NULL: every particle is a member).  *n_members = m; with m == 0 no source
 * entry is written.  PFMPE_E_ARG for a NULL source with n_new > 0, a NULL n_members, N < 0, n_new < 0, N or n_new above
 * 2^31 - 1, a mode outside 0..255 when mode_of is given; the outputs are untouched then. */
int pfmpe_host_resample_source(const uint8_t* mode_of /* N bytes; NULL: all members */, int64_t N, int32_t mode,
                               int64_t n_new, int32_t* source /* n_new */, int64_t* n_members);
/* host-only: the rank r of the one slot k by the function the device runs.  PFMPE_E_ARG for a NULL rank, m < 1,
 * n_new < 1, k outside 0..n_new-1, m or n_new above 2^31 - 1; *rank is untouched then. */
int pfmpe_host_resample_rank(int64_t k, int64_t m, int64_t n_new, int64_t* rank);

/* ------------------------------------------------------------- LED-blob association of the particle cloud */
/* The reference keeps the correspondences of every particle (correspondencesVec, PE:2385-2445, read at PE:688); a
 * step reports the winner's only (pfmpe_frame_out.corr).  These calls derive every particle's pairs on the device
 * and return them as rows, or counted: which blob each LED matched, over the whole set.
 *
 * Sets.  `which` as for pfmpe_get_particles: PFMPE_ASSOC_PROPAGATED the kept propagated set of the last step
 * (the set correspondencesVec belongs to), PFMPE_ASSOC_POSTERIOR the current prior (the resampled set).  Every
 * particle casts one vote per LED; weights are not used (the posterior carries them as multiplicities), so every
 * number is an integer and a repeated call returns the same bits.
 *
 * Definition.  The pairs of particle i are those the step's likelihood lists for pose i in the context's compute
 * type (fp64 for F64 state, fp32 for F32 / F16 state), with the poses pfmpe_get_particles(which) returns, the blobs
 * given here and the context's current tol, tol_PF, model, K and pruning option: LED j's nearest blob (lowest blob
 * index on a tie); extraction in ascending (distance, LED) order; the reference's break at the first distance above
 * tol_PF and at most min(B, M) pairs; LEDs used once, blobs free to repeat; 1-based (LED, blob) rows padded with
 * zeros to PFMPE_MAX_MARKERS rows as in pfmpe_frame_out.corr; no pairs for a particle whose likelihood
 * short-circuits (B = 0, a NaN distance at LED 1 / blob 1).
 * votes[m * (B + 1) + b], b >= 1, counts the particles that paired LED m + 1 with blob b; column 0 counts those that
 * left LED m + 1 unpaired, so every row sums to n.
 *
 * Blobs are the caller's (the context keeps no frame's list): a host list, or a frame of the staged blob bank.
 * Both device calls are blocking, run on the context's stream, change nothing a later frame reads and are not timed
 * by PFMPE_OPT_TIMING (regenerating the propagated set counts as aux, as for the particle read-back).
 * Errors: PFMPE_E_ARG for a bad `which`, a NULL in / out, NULL blobs with B > 0 and no bank frame, B < 0, a bank
 * frame out of range, first < 0, count < 0 or first + count > N, NULL corr / n_corr with count > 0; PFMPE_E_CAP for
 * B > max_blobs; PFMPE_E_STATE without a model or a particle set, and for PROPAGATED before the first step. */
enum { PFMPE_ASSOC_PROPAGATED = 0, PFMPE_ASSOC_POSTERIOR = 1 };
typedef struct {
  const double* blobs;  /* B x 2 undistorted px, host pointer (ignored if bank_frame >= 0)          */
  int32_t B;            /* (a bank frame brings its own count, returned in out->B; B < 0 is refused) */
  int32_t bank_frame;   /* -1: use `blobs`; >= 0: that frame of the staged blob bank               */
} pfmpe_assoc_in;
typedef struct {
  int64_t n;                                   /* particles examined (= every LED row's vote total)  */
  int32_t M, B;                                /* shape of the votes table                           */
  int64_t n_any;                               /* particles with at least one pair                   */
  uint32_t matched[PFMPE_MAX_MARKERS];         /* n - votes[m][0]                                    */
  uint32_t mode_blob[PFMPE_MAX_MARKERS];       /* 1-based blob with the most votes of LED m (lowest
                                                  index on a tie); 0 when no particle matched LED m   */
  uint32_t mode_votes[PFMPE_MAX_MARKERS];
  uint32_t second_votes[PFMPE_MAX_MARKERS];    /* votes of the runner-up blob (0 if none)            */
  uint32_t npairs_hist[PFMPE_MAX_MARKERS + 1]; /* particles with exactly k pairs                     */
  uint32_t pad;
} pfmpe_assoc_out;                             /* 352 bytes */
/* votes: M x (B + 1) words, row-major, may be NULL.  (Runs as pfmpe_assoc_stats_multi, below, with one entry: one
 * path, one kernel and one scratch for both.) */
int pfmpe_assoc_stats(pfmpe_ctx* ctx, int which, const pfmpe_assoc_in* in, pfmpe_assoc_out* out, uint32_t* votes);
/* the rows of particles first .. first + count - 1 (the reference's correspondencesVec[i]):
 * corr count x 2*PFMPE_MAX_MARKERS words, n_corr count pair counts */
int pfmpe_get_pairs(pfmpe_ctx* ctx, int which, const pfmpe_assoc_in* in, int64_t first, int32_t count,
                    uint32_t* corr, int32_t* n_corr);

#define PFMPE_ASSOC_MAX_STREAMS 64
#define PFMPE_ASSOC_MAX_LAUNCHES 16   /* 2 sets x 4 marker buckets x 2 pruning options */

/* pfmpe_assoc_stats for S entries (the votes of every object of a frame, the numUAV loop, PE:89) as one launch
 * sequence with one synchronise: one upload of all blob tables and descriptors, one memset of all bins, one votes
 * launch per kernel instance the batch needs, one read-back into pinned memory, one synchronise.  out[s] and votes[s]
 * are byte for byte what pfmpe_assoc_stats(ctxs[s], in[s].which, &in[s].blobs, &out[s], votes[s]) writes; votes = NULL
 * or votes[s] = NULL: that table is not wanted, otherwise votes[s] holds M_s x (B_s + 1) words.  Every number is an
 * integer sum, so this holds whatever grid the batch uses.
 * Per entry: its own `which`, blob list and B.  M, the markers, K, tol, tol_PF, the pruning option, N and the prior's
 * storage (particle order or owner indices, fp16 anchor) are its context's.  A context may appear in several entries
 * (both sets of one object, or two blob lists); a context with at least one PROPAGATED entry regenerates its kept set
 * once, on its own stream, and all its entries read that set.  Contexts: on one device, of one state type; pruning
 * options and marker counts may differ (entries are grouped into launches by set, marker bucket and pruning option).
 * Runs on ctxs[0]'s stream in scratch ctxs[0] owns (grown on demand, never shrunk); ctxs[0] receives the error text;
 * work a member has pending elsewhere (its regeneration included) is ordered before the batch; blocking.  Reads only:
 * no context's state, staged table use or statistics change, except that a member's regeneration counts as aux on that
 * member.  Not timed by PFMPE_OPT_TIMING.  DESIGN.md §4.12a: design, resources and measured times.
 * Everything is checked before anything is staged, regenerated or launched, and out / votes are untouched on an error:
 * PFMPE_E_ARG (S < 1, NULL ctxs / in / out / ctxs[s], a device or state-type mismatch, a bad `which`, B < 0, NULL blobs
 * with B > 0 and no bank frame, a bank frame out of range), PFMPE_E_CAP (S > PFMPE_ASSOC_MAX_STREAMS, an entry's B above
 * its context's max_blobs, a blob table that exceeds the LDS, as the single call), PFMPE_E_STATE (an entry whose context
 * has no model or no particle set, PROPAGATED before that context's first step); the text begins
 * "assoc_stats_multi: stream <s>: ".  With ctxs == NULL or ctxs[0] == NULL: PFMPE_E_ARG and no text. */
typedef struct {
  pfmpe_assoc_in blobs;   /* this entry's list: host pointer + B, or a frame of ITS context's staged bank */
  int32_t which;          /* PFMPE_ASSOC_PROPAGATED / PFMPE_ASSOC_POSTERIOR */
  int32_t pad;
} pfmpe_assoc_multi_in;   /* 24 bytes */
int pfmpe_assoc_stats_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_assoc_multi_in* in,
                            pfmpe_assoc_out* out, uint32_t* const* votes);

/* host-only (no GPU, no context): the layout of a pfmpe_assoc_stats_multi batch, which the call stages exactly.  Entry
 * s has N[s] particles, M[s] LEDs, B[s] blobs, the set which[s] (NULL: all POSTERIOR) and the pruning option prune[s]
 * (NULL: all on) in a batch of contexts of state_dtype.  Per entry: blocks = min(ceil(N / 256), 1024), the single
 * call's grid; launch, the index of its launch (entries of one set, marker bucket (M = 5; <= 8; <= 12; <= 16) and
 * pruning option share a launch; launches are numbered in order of first appearance); first_block, the running sum of
 * blocks over the earlier entries of that launch; bins_offset, in words, of its M * B + M + 1 bins in the one device
 * table (entries follow each other in index order, each start rounded up to 4 words); lds_votes = 1 when table + 16
 * bytes + bins + the kernel's constants fit the workgroup's 64 KiB of LDS, the single call's rule, else 0 (its votes
 * then go straight into the device table; M = 16 with B = 1024 is such an entry).  The size of an fp32 blob table
 * depends on the blob positions (its cell grid): table_bytes[s] gives the built table's size, as the call does; with
 * table_bytes = NULL the size of a table without a grid is taken (every fp64 table, every table with B = 0).
 * total: the bins' word count, the launches, and the blocks of each launch's flat grid.
 * PFMPE_E_ARG for a NULL N / M / B / plan / total, S < 1, a bad state_dtype, N < 1, M outside 1..PFMPE_MAX_MARKERS, B < 0,
 * a bad which, a negative table size; PFMPE_E_CAP for S > PFMPE_ASSOC_MAX_STREAMS, B > PFMPE_MAX_BLOBS or a table that
 * does not fit the LDS at all; the outputs are untouched then. */
typedef struct {
  int64_t bins_offset;
  int32_t first_block, blocks, launch, lds_votes;
} pfmpe_assoc_plan;         /* 24 bytes */
typedef struct {
  int64_t bins_words;
  int32_t launches, pad;
  int32_t launch_blocks[PFMPE_ASSOC_MAX_LAUNCHES];
} pfmpe_assoc_plan_total;   /* 80 bytes */
int pfmpe_host_assoc_plan(const int32_t* N, const int32_t* M, const int32_t* B, const int32_t* which /* may be NULL */,
                          const int32_t* prune /* may be NULL */, const int32_t* table_bytes /* may be NULL */, int S,
                          int state_dtype, pfmpe_assoc_plan* plan, pfmpe_assoc_plan_total* total);

/* host-only (no GPU, no context): gating a row of pairs (the winner's, pfmpe_frame_out.corr) by the support a votes
 * table (pfmpe_assoc_stats, M x (B + 1)) gives it, before the row goes to Gauss-Newton.  n is row 0's sum.  For row
 * k = (led, blob) of corr, in order: v = votes[led-1][blob], and (mode_blob, mode_votes, second_votes) of that LED as
 * pfmpe_host_assoc_summary forms them.  reason[k] has bit 0 set when !((double)v >= min_share * (double)n), bit 1 when
 * mode_blob != blob, bit 2 when lead * (double)second_votes > (double)mode_votes.  A row with reason[k] == 0 is kept,
 * in order; n_gated counts them.  fallback = 1 when n_gated < min_pairs: then gated is the input row unchanged (the
 * first n_corr pairs, zero padded) and the caller may skip Gauss-Newton; otherwise gated holds the kept rows and
 * zeros.  Defaults: min_share 0.5, lead 2.0, min_pairs 4 (the reference's min_num_leds_detected_,
 * pose_estimator.h:104).  reason[k] is 0 for k >= n_corr.
 * PFMPE_E_ARG for a NULL votes / corr / gated / out, M outside 1..PFMPE_MAX_MARKERS, B outside 0..PFMPE_MAX_BLOBS, n_corr
 * outside 0..PFMPE_MAX_MARKERS, an LED index outside 1..M or a blob index outside 1..B in the first n_corr rows, rows
 * of votes that do not all sum to n, a NaN, negative or infinite min_share or lead, min_pairs < 0; the outputs are
 * untouched then. */
typedef struct { double min_share; double lead; int32_t min_pairs; int32_t pad; } pfmpe_gate_params;   /* 24 bytes */
typedef struct { int32_t n_in, n_gated, fallback, pad; uint8_t reason[PFMPE_MAX_MARKERS]; } pfmpe_gate_out; /* 32 bytes */
void pfmpe_default_gate_params(pfmpe_gate_params* p);   /* 0.5, 2.0, 4 */
int pfmpe_host_gate_pairs(const uint32_t* votes, int M, int B, const uint32_t* corr /* 2*PFMPE_MAX_MARKERS */,
                          int n_corr, const pfmpe_gate_params* params /* NULL: defaults */,
                          uint32_t* gated /* 2*PFMPE_MAX_MARKERS, zero padded */, pfmpe_gate_out* out);

/* ------------------------------------------------------------- the K best distinct hypotheses of a frame */
/* A step names two particles (the most likely one, the most resampled one); the runner-up, the mirror solution LED
 * markers are known for (the reference's checkAmbiguity / correspondencesVec), had to be found on the host from
 * pfmpe_get_weights and pfmpe_get_particles(0).  pfmpe_top_particles ranks the cloud on the device and returns the K
 * best rows, optionally thinned so that no two of them are the same mode; its poses / corr feed pfmpe_refine_poses.
 *
 * Set: the kept propagated set of the last step, the rows of pfmpe_get_particles(0).  Key: PFMPE_TOP_BY_WEIGHT the
 * kept iteration's raw weight (the particle's value in pfmpe_get_weights), PFMPE_TOP_BY_COUNT its resample count
 * (pfmpe_get_counts).  Eligible: key > 0 (never a zero or NaN weight, never a zero count).  Ranking: larger key
 * first, the lower particle index first among equal keys (the reference's first-max rule, maxCoeff, extended to K): a
 * total order, so a repeated call returns the same bytes.
 * Without suppression (min_trans == 0 and min_rot == 0) the rows are the first min(K, n_positive) of the ranking.
 * With suppression the pool, the first min(PFMPE_TOP_POOL, n_positive) of the ranking, is walked in rank order:
 * candidate j is kept unless an already kept candidate i is near it; the walk stops when K are kept or the pool ends;
 * n_examined counts the candidates walked.  Near = near_t and near_r, in fp64 on the 12-double poses, every product and
 * sum rounded on its own, left to right:
 *   d2 = (tj0-ti0)^2 + (tj1-ti1)^2 + (tj2-ti2)^2;             near_t: min_trans == 0 or d2 < min_trans*min_trans
 *   tr = sum of Rj[r][c]*Ri[r][c] over the nine entries, row-major;  near_r: min_rot == 0 or tr > 1 + 2*cos(min_rot)
 * (a threshold of 0 does not separate; the right-hand sides are formed once on the host).
 *
 * Outputs, all optional but `out`: index[r] the particle index of row r, key_value[r] its key as a double, poses the
 * rows pfmpe_get_particles(0) holds for these indices, corr / n_corr the rows
 * pfmpe_get_pairs(PFMPE_ASSOC_PROPAGATED, blobs, index[r], 1) returns (only when blobs is not NULL).  Exactly n_out
 * rows of each array are written, nothing else of them is touched.
 * The call blocks, runs on the context's stream, changes nothing a later frame reads, moves no per-particle array to
 * the host and is not timed by PFMPE_OPT_TIMING (regenerating the pool's poses counts as aux).
 * Errors, checked before anything is launched (the outputs stay untouched): PFMPE_E_ARG for a NULL ctx, params or
 * out, a bad key, K outside 0..PFMPE_TOP_MAX, a negative or non-finite min_trans, min_rot outside [0, pi] or NaN, a
 * blob descriptor pfmpe_get_pairs refuses; PFMPE_E_CAP for B > max_blobs; PFMPE_E_STATE before the first step, for
 * BY_COUNT with PFMPE_OPT_RECORD_COUNTS off or after a step that did not resample (as pfmpe_get_counts), and for
 * blobs without a model. */
#define PFMPE_TOP_MAX  1024   /* largest K */
#define PFMPE_TOP_POOL 1024   /* ranked candidates the suppression walks */
enum { PFMPE_TOP_BY_WEIGHT = 0, PFMPE_TOP_BY_COUNT = 1 };
typedef struct {
  int32_t key;        /* PFMPE_TOP_BY_*                                    */
  int32_t K;          /* rows wanted, 0 .. PFMPE_TOP_MAX                    */
  double  min_trans;  /* m,   >= 0, finite; 0: translation does not separate */
  double  min_rot;    /* rad, 0 .. pi;      0: rotation does not separate    */
} pfmpe_top_params;   /* 24 bytes */
typedef struct {
  int64_t n;           /* particles ranked (N)                              */
  int64_t n_positive;  /* particles with key > 0 (the eligible ones)        */
  int32_t n_out;       /* rows written                                      */
  int32_t n_examined;  /* ranked candidates walked (== n_out without suppression) */
} pfmpe_top_out;       /* 24 bytes */
void pfmpe_default_top_params(pfmpe_top_params* p);   /* BY_WEIGHT, K = 8, 0, 0 */
/* blobs NULL: no pairs; poses K x 12, corr K x 2*PFMPE_MAX_MARKERS, index / key_value / n_corr K */
int pfmpe_top_particles(pfmpe_ctx* ctx, const pfmpe_top_params* params, const pfmpe_assoc_in* blobs, pfmpe_top_out* out,
                        int32_t* index, double* key_value, double* poses, uint32_t* corr, int32_t* n_corr);
/* The suppression walk alone, on the host, for P caller-given poses already in rank order (P >= 0, may exceed
 * PFMPE_TOP_POOL): the predicate is the function the device runs.  keep (K) receives positions within the list.
 * PFMPE_E_ARG for a NULL pointer, P < 0, K outside 0..PFMPE_TOP_MAX, a bad threshold or a non-finite pose. */
int pfmpe_host_top_suppress(const double* poses, int32_t P, int32_t K, double min_trans, double min_rot,
                            int32_t* keep, int32_t* n_out, int32_t* n_examined);

/* ------------------------------------------------------------------- Gauss-Newton refinement of hypotheses */
/* Replaces PoseEstimator::optimisePose (PE:1805-2009): the reference refines the winner of the PF step over its
 * correspondences and publishes that pose and pose_covariance_ = A.inverse() (PE:2004).  pfmpe_refine_poses does so
 * for K caller-given hypotheses (K = 1 with pfmpe_frame_out.most_likely_pose / .corr is the reference's step);
 * pfmpe_refine_cloud refines every particle of a set from its own pairs, one lane per particle, and names the best.
 *
 * Definition, per hypothesis, fp64 for every state type (the formulas of PE:1805-2009 in their order, unfused):
 * at most max_iter iterations; rows with blob index 0 are skipped; per pair e = z - project2d(pose, LED) through the
 * full K (PE:1017-1034) and the 2 x 6 Jacobian of computeJacobian (PE:2163-2192) on the camera-frame point with
 * fx = K[0], fy = K[4]; A += J^T J, b += J^T e in row order; dT = A.ldlt().solve(b) with Eigen's symmetric diagonal
 * pivoting (dT = 0 when a pivot is exactly 0); pose = exponentialMap(dT) * pose (PE:2194-2226); stop when
 * max |dT| <= converged.  At the last allowed iteration the reference's rule (PE:1886-1895) with its `=+`: e_init and
 * e_end are the error norms of the last used pair at iteration 0 and at the last iteration, and the start pose is
 * restored when e_init < e_end.  The covariance is the inverse of the last A formed, column by column through the
 * same factors, all zeros when a pivot was 0.  rms_before / rms_after = sqrt(mean |z - uv|^2) over the used pairs at
 * the start pose and at the returned pose (not computed by the reference).
 * The iteration count is not stable: convergence ends in rounding noise around `converged`, so a change of one ulp
 * in the start pose moves it, also across max_iter.  The refined pose of a converged hypothesis is stable.
 *
 * CLOUD: hypothesis i is particle first + i of set `which` (PFMPE_ASSOC_PROPAGATED / _POSTERIOR): its start pose is
 * the 12 doubles pfmpe_get_particles(which) returns for it, its rows those pfmpe_get_pairs(which) returns for it.
 * The summary always covers all N particles; rows / cov cover the requested range.
 * Best hypothesis: most pairs, then the smallest rms_after, then the lowest index, among those with at least one pair
 * and a finite rms_after.  Every number of the summary is an integer or belongs to one hypothesis: a repeated call
 * returns the same bits.
 *
 * Both device calls are blocking, run on the context's stream, change nothing a later frame reads and are not timed
 * by PFMPE_OPT_TIMING (regenerating the propagated set counts as aux, as for the particle read-back).  params NULL:
 * the defaults.  K = 0 / count = 0 are valid (CLOUD: the summary still covers all N).
 * Errors: PFMPE_E_ARG for a NULL out or blobs descriptor, NULL blobs with B > 0 and no bank frame, B < 0, a bank
 * frame out of range, NULL poses / corr with K > 0, K < 0, an LED index above M (or 0 beside a blob) or a blob index
 * above B in corr, a non-finite start pose, a bad `which`, first < 0, count < 0 or first + count > N, max_iter
 * outside 1..10000, a negative or NaN converged; PFMPE_E_CAP for B > max_blobs or K > max_particles; PFMPE_E_STATE
 * without a model, CLOUD without a particle set, and for PROPAGATED before the first step. */
typedef struct {
  int32_t max_iter;             /* 500  (PE:1810), 1..10000                                        */
  int32_t revert_on_divergence; /* 1    (PE:1886-1892); 0 keeps the last iterate                   */
  double  converged;            /* 1e-13 (PE:1809), >= 0                                           */
} pfmpe_refine_params;
void pfmpe_default_refine_params(pfmpe_refine_params* p);

enum { PFMPE_REFINE_NO_PAIRS = 0, PFMPE_REFINE_CONVERGED = 1, PFMPE_REFINE_CAP_KEPT = 2, PFMPE_REFINE_CAP_REVERTED = 3 };
typedef struct {
  double pose[12];              /* refined pose; the start pose for NO_PAIRS / CAP_REVERTED         */
  double rms_before, rms_after; /* px; 0 for NO_PAIRS                                               */
  int32_t iters;                /* PubData.numIter when converged, else max_iter                    */
  int32_t n_pairs;              /* rows used (blob != 0)                                            */
  int32_t status, pad;
} pfmpe_refine_row;             /* 128 bytes */

typedef struct {
  int64_t n, n_with_pairs, n_converged, n_cap_kept, n_cap_reverted;
  int64_t iters_total; int32_t iters_max; int32_t pad;
  int64_t best;                 /* index within the call (LIST: row; CLOUD: particle index), -1 if none */
  pfmpe_refine_row best_row;
  double best_cov[36];          /* pose_covariance_ = A.inverse() (PE:2004) of the best hypothesis  */
} pfmpe_refine_out;

/* optimisePose for K caller-given hypotheses: poses K x 12, corr K x 2*PFMPE_MAX_MARKERS (1-based (LED, blob)
 * rows, zero padded, as pfmpe_frame_out.corr).  rows (K) and cov (K x 36) may be NULL. */
int pfmpe_refine_poses(pfmpe_ctx* ctx, const pfmpe_assoc_in* blobs, const pfmpe_refine_params* params,
                       const double* poses, const uint32_t* corr, int32_t K, pfmpe_refine_out* out,
                       pfmpe_refine_row* rows, double* cov);
/* every particle of set `which` (PFMPE_ASSOC_PROPAGATED / _POSTERIOR) from its own pairs; the summary covers all
 * N, rows / cov (may be NULL) cover particles first .. first + count - 1 */
int pfmpe_refine_cloud(pfmpe_ctx* ctx, int which, const pfmpe_assoc_in* blobs, const pfmpe_refine_params* params,
                       int64_t first, int32_t count, pfmpe_refine_out* out, pfmpe_refine_row* rows, double* cov);
#define PFMPE_REFINE_MAX_STREAMS 64
#define PFMPE_REFINE_MULTI_MAX_HYPOTHESES 65536   /* all streams together: one chunk */
#define PFMPE_REFINE_DESC_BYTES 48                /* a stream's descriptor in the upload buffer (the plan below) */

/* pfmpe_refine_poses for S streams as one batch (the numUAV loop's optimisePose, PE:89: the winner of every accepted
 * object of a frame): one upload of one packed buffer, one Gauss-Newton launch over all hypotheses, one launch that
 * folds every stream's summary, one read-back and one synchronise, where S single calls make S of each sequence.
 * out[s], rows[s] and cov[s] are byte for byte what
 *   pfmpe_refine_poses(ctxs[s], &in[s].blobs, &params[s], in[s].poses, in[s].corr, in[s].K, &out[s], rows[s], cov[s])
 * writes (out[s].n = K_s, best an index within the stream, the zeroed best_row / best_cov when no hypothesis is
 * eligible, the empty summary for K_s = 0): a lane runs the same function on the same numbers, every summed quantity
 * is an integer and the best key is a total order.  Per stream: M, the markers and K (from its context), its blob
 * list and B, K_s and every field of params[s] (params = NULL: the defaults for all, else S records).  rows = NULL or
 * rows[s] = NULL, cov = NULL or cov[s] = NULL: not wanted, else K_s rows / K_s x 36.
 * Contexts of any state types may be mixed; they must be on one device; a context may appear more than once (two blob
 * lists of one camera).  The call reads only a member's model and the host copy of its blob bank: no member's device
 * state is read or written, so nothing is ordered with the members' own streams.  ctxs[0] leads: the batch runs on
 * its stream, in a scratch buffer and a pinned staging block it owns (grown on demand, never shrunk), and it receives
 * the error text.  Blocking; not timed by PFMPE_OPT_TIMING.
 * Everything is checked before anything is staged or launched; on an error out, rows and cov are untouched and no
 * context changes: PFMPE_E_ARG (S < 1, NULL ctxs / in / out / ctxs[s], a device mismatch, K_s < 0, NULL poses / corr
 * with K_s > 0, B < 0, NULL blobs with B > 0 and no bank frame, a bank frame out of range, an LED or blob index out of
 * range, a non-finite start pose, bad params[s]), PFMPE_E_CAP (S > PFMPE_REFINE_MAX_STREAMS, B_s > max_blobs of
 * ctxs[s], K_s > max_particles of ctxs[s], the sum of K_s above PFMPE_REFINE_MULTI_MAX_HYPOTHESES), PFMPE_E_STATE (a
 * stream without a model); the text, "refine_multi: stream <s>: ...", is the last-error text of ctxs[0].  With
 * ctxs = NULL or ctxs[0] = NULL: PFMPE_E_ARG, no text. */
typedef struct {
  pfmpe_assoc_in blobs;   /* this stream's blob list: host pointer + B, or a frame of ITS context's staged bank */
  const double* poses;    /* K x 12 start poses; may be NULL when K == 0 */
  const uint32_t* corr;   /* K x 2*PFMPE_MAX_MARKERS pair rows, as pfmpe_frame_out.corr; may be NULL when K == 0 */
  int32_t K;              /* hypotheses of this stream; 0 is valid (the object was not accepted this frame) */
  int32_t pad;
} pfmpe_refine_in;        /* 40 bytes */
int pfmpe_refine_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_refine_in* in, const pfmpe_refine_params* params,
                       pfmpe_refine_out* out, pfmpe_refine_row* const* rows, double* const* cov);

/* host-only (no GPU, no context): the packed upload buffer of the batch, which the call above stages exactly.  With
 * H = sum of K the buffer holds, each region 16-byte aligned, disjoint from the others and inside [0, upload_bytes):
 * S descriptors of PFMPE_REFINE_DESC_BYTES, the stream index of every hypothesis (H int32), the start poses
 * (H x 12 doubles), the pair rows (H x 2*PFMPE_MAX_MARKERS words), and per stream its model (PFMPE_MAX_MARKERS x 3
 * doubles of markers, then the 9 of K) and its blobs (2 * B doubles).  The layout depends on K, B and S alone.
 * download_bytes: the summaries (S), rows (H) and covariances (H x 36) the device writes behind the upload.
 * PFMPE_E_ARG for a NULL pointer, S < 1, K < 0 or B < 0; PFMPE_E_CAP for S > PFMPE_REFINE_MAX_STREAMS,
 * B > PFMPE_MAX_BLOBS or H > PFMPE_REFINE_MULTI_MAX_HYPOTHESES; the outputs are untouched then. */
typedef struct {
  int64_t first;         /* index of the stream's first hypothesis in the batch: prefix sum of K */
  int64_t model_offset;  /* byte offset in the upload buffer of its markers (PFMPE_MAX_MARKERS x 3 doubles) + K (9) */
  int64_t blobs_offset;  /* byte offset of its 2 * B doubles (any valid offset when B == 0) */
} pfmpe_refine_plan;     /* 24 bytes */
typedef struct {
  int64_t hypotheses;                                   /* sum of K */
  int64_t desc_offset, stream_of_offset, poses_offset, corr_offset;  /* S descriptors; H int32; H x 12 doubles; H x 32 words */
  int64_t upload_bytes, download_bytes;
} pfmpe_refine_plan_total;                              /* 56 bytes */
int pfmpe_host_refine_plan(const int32_t* K, const int32_t* B, int S, pfmpe_refine_plan* plan,
                           pfmpe_refine_plan_total* total);

/* host-only: the same __host__ __device__ code for one hypothesis (no GPU, no context).  corr: n_rows rows (any
 * count).  PFMPE_E_ARG for a NULL pointer, M < 1, B < 0, n_rows < 0, a bad index, a non-finite start pose or bad
 * parameters, as above.  params may be NULL, cov36 may be NULL. */
int pfmpe_host_optimise_pose(const double* markers_xyz, int M, const double* K, const double* blobs, int B,
                             const uint32_t* corr, int n_rows, const pfmpe_refine_params* params, const double* pose12,
                             pfmpe_refine_row* row, double* cov36);

/* The step and the refinement of its winner in one blocking call: every accepted frame of the reference ends with
 * optimisePose on the step's winner (PE:687-690), which pfmpe_step followed by pfmpe_refine_poses does with two host
 * round trips.  Here a one-wave kernel (k_step_tail) runs behind every launch that can finish the frame, on the
 * frame's stream: it takes the winner pose and its pair row from the frame record where the device left it, runs the
 * Gauss-Newton of pfmpe_refine_poses on them and publishes the result as the step publishes its record; the host
 * waits once.  The fp64 blobs (the caller's list, or the bank frame's host copy), the model and the parameters are
 * staged in a mapped pinned block of the context (grown on demand, never shrunk) that the host writes once per call;
 * no copy command is issued.
 * Defined by equivalence: `out` and the context's state afterwards are those of pfmpe_step(ctx, in, out).  With
 * out->flag_fail == PFMPE_FLAG_ACCEPTED and a finite winner pose, gn, row and cov36 are byte for byte what
 *   pfmpe_refine_poses(ctx, {in->blobs, in->B, in->bank_frame}, params, out->winner_pose, out->corr, 1, gn, row, cov36)
 * writes; otherwise (a rejected frame, a non-finite winner pose) gn is that call's K = 0 summary (n = 0, best = -1,
 * zeroed best_row and best_cov) and row and cov36 are not written.  row and cov36 may be NULL; params NULL: the
 * defaults.  params is checked by pfmpe_refine_poses' rules, and `in` by pfmpe_step's, before anything is staged or
 * launched: on an error no context changes.  With PFMPE_OPT_TIMING the tail is one more PFMPE_K_AUX bracket (on a
 * one-launch frame: the tail alone).
 * A tail that finds no finished record of its frame is never an error: the call then refines through
 * pfmpe_refine_poses' own path, returns the same bytes and counts it in PFMPE_INFO_TAIL_FALLBACKS. */
int pfmpe_step_refine(pfmpe_ctx* ctx, const pfmpe_frame_in* in, const pfmpe_refine_params* params,
                      pfmpe_frame_out* out, pfmpe_refine_out* gn, pfmpe_refine_row* row, double* cov36);
/* The batch: pfmpe_step_multi with every stream's tail in one launch per round, one wave per stream.  Stream s gets
 * exactly what pfmpe_step_refine(ctxs[s], &in[s], &params[s], &out[s], &gn[s], &rows[s], &cov[36 * s]) gives (params
 * NULL or S records, rows NULL or S rows, cov NULL or S x 36 doubles; the row and the covariance of a stream that is
 * not refined are not written).  Limits, member rules, ordering and errors are pfmpe_step_multi's, the texts begin
 * "step_refine_multi: stream <s>: "; ctxs[0] leads and owns the staging block. */
int pfmpe_step_refine_multi(pfmpe_ctx* const* ctxs, int S, const pfmpe_frame_in* in, const pfmpe_refine_params* params,
                            pfmpe_frame_out* out, pfmpe_refine_out* gn, pfmpe_refine_row* rows, double* cov);
/* host-only (no GPU, no context): the tail's own __host__ __device__ code for a caller-given finished frame, blobs
 * B x 2.  PFMPE_E_ARG for a NULL pointer (row, cov36 and params may be NULL), M outside 1..PFMPE_MAX_MARKERS, B < 0,
 * bad parameters, or an index of frame->corr out of range in a frame that is refined. */
int pfmpe_host_step_tail(const double* markers_xyz, int M, const double* K, const double* blobs, int B,
                         const pfmpe_frame_out* frame, const pfmpe_refine_params* params, pfmpe_refine_out* gn,
                         pfmpe_refine_row* row, double* cov36);

/* Engine options (value semantics in brackets; defaults first):
 *   PFMPE_OPT_RECORD_COUNTS [0|1]  keep counterMeas on device for pfmpe_get_counts
 *   PFMPE_OPT_PRUNE         [1|0]  exact x-window blob pruning in the likelihood (0 = scan all B blobs)
 *   PFMPE_OPT_TIMING        [0|P]  bracket the kernel launches of every P-th frame with HIP events
 *                                  (pfmpe_get_kernel_stats); P = 1 times every frame, 0 is off
 *   PFMPE_OPT_FUSED         [2|1|0] run a frame as ONE launch whenever all its blocks fit on the device
 *                                  at once: 2 (default) k_frame2 with flat hand-offs (every block reduces
 *                                  all block partials itself; <= 512 blocks), 1 k_frame with tree
 *                                  hand-offs; 0 forces the two-launch path (k_propagate_weigh + k_resample)
 *   PFMPE_OPT_KEEP_PROPAGATED [1|0] two-launch path: k_propagate_weigh stores each iteration's propagated
 *                                  set (two extra state buffers, allocated on first use) and k_resample
 *                                  gathers from it; 0 regenerates the kept set in k_resample instead.
 *                                  Results are bit-identical either way.  Default 1; batched frames
 *                                  (pfmpe_step_multi) use the stored set for fp16 state only (measured)
 *   PFMPE_OPT_WAIT_BOUND_US [2000000|>=1] bound of every in-launch wait of a one-launch frame.  A frame whose
 *                                  blocks are not all resident (other work holding CUs) is abandoned at the
 *                                  bound, redone with two launches (same result) and one-launch frames are
 *                                  switched off on this context (PFMPE_INFO_FUSED_FALLBACKS counts it;
 *                                  pfmpe_last_error describes it, the step still returns PFMPE_OK)
 *   PFMPE_OPT_FUSED_REARM   [0|n]  after such a fallback, switch one-launch frames back on after n clean
 *                                  two-launch frames (0: stay off)
 *   PFMPE_OPT_MULTI_MAX_BLOCKS [160000|1..160000] largest pfmpe_step_multi batch this context leads, in
 *                                  256-particle blocks (PFMPE_E_CAP above); the default is the tested limit
 *   PFMPE_OPT_DEFER_RESAMPLE [1|0] two-launch frames with the kept propagated set: resampling writes each
 *                                  slot's owner index (4 B) instead of gathering and scattering the particle,
 *                                  and the next frame reads the prior through those indices.
 *                                  Results are bit-identical either way (pfmpe_get_particles gathers)
 * Within one process at most one one-launch frame runs per device at a time: a context that finds another
 * context's one-launch frame in flight on its device runs that frame as two launches (PFMPE_INFO_GUARD_SKIPS). */
enum { PFMPE_OPT_RECORD_COUNTS = 1, PFMPE_OPT_PRUNE = 2, PFMPE_OPT_TIMING = 3, PFMPE_OPT_FUSED = 4,
       PFMPE_OPT_KEEP_PROPAGATED = 5, PFMPE_OPT_WAIT_BOUND_US = 6, PFMPE_OPT_FUSED_REARM = 7,
       PFMPE_OPT_MULTI_MAX_BLOCKS = 8, PFMPE_OPT_DEFER_RESAMPLE = 9 };
int pfmpe_set_option(pfmpe_ctx* ctx, int option, int64_t value);

/* Context state for monitoring and tests (no reference counterpart: engine introspection). */
enum { PFMPE_SHAPE_TWO_LAUNCH = 0, /* weighing pass (+ re-launches) + hand-off + resampling (+ final)   */
       PFMPE_SHAPE_FRAME = 1,      /* k_frame: one launch, tree hand-offs                                */
       PFMPE_SHAPE_FRAME2 = 2 };   /* k_frame2: one launch, flat hand-offs                               */
enum { PFMPE_INFO_FUSED = 1,            /* current one-launch mode (0/1/2; 0 after a fallback)       */
       PFMPE_INFO_FUSED_FALLBACKS = 2,  /* one-launch frames abandoned at the wait bound and redone  */
       PFMPE_INFO_LAST_SHAPE = 3,       /* PFMPE_SHAPE_* of the last step (-1 before the first)      */
       PFMPE_INFO_GUARD_SKIPS = 4,      /* frames run as two launches because another was in flight  */
       PFMPE_INFO_N = 5,                /* current particle count                                    */
       PFMPE_INFO_LAST_WEIGH_PASS = 6,  /* PFMPE_WEIGH_* of the last two-launch weighing (-1: none)  */
       PFMPE_INFO_LAST_GRID = 7,        /* 1: the last frame's blob table searched its cell grid; 0: the
                                         * x-buckets (no grid for this table or its window; fp64)    */
       PFMPE_INFO_LAST_RESAMPLE = 8,    /* PFMPE_RESAMPLE_* of the last two-launch resampling (-1: none) */
       PFMPE_INFO_NUM_CU = 9,           /* compute units of the context's device (pfmpe_host_init_plan's num_cu) */
       PFMPE_INFO_TAIL_FALLBACKS = 10 };/* pfmpe_step_refine(_multi) frames of this context refined by the recovery path */
/* The two-launch shape's weighing pass: one block per 256 particles (k_propagate_weigh), or
 * resident blocks streaming over them with the next block's state prefetched (k_weigh_stream + k_group +
 * k_top), or the streaming pass with two particles per lane in packed fp32 (k_weigh_pk: 5 markers, fp32 / fp16
 * state; k_weigh_pk12: 12 markers, fp32 state; the Philox stream, the blob grid).  All give bit-identical
 * results. */
enum { PFMPE_WEIGH_BLOCKS = 0, PFMPE_WEIGH_STREAM = 1, PFMPE_WEIGH_PK = 2 };
/* The two-launch shape's resampling launch: one block per 256 particles with the new prior materialised
 * (k_resample, then k_resample_final), or, for a deferred frame, one wave per 256-particle block writing owner
 * indices whose last wave finishes the frame (k_resample_owners).  Same outputs. */
enum { PFMPE_RESAMPLE_BLOCKS = 0, PFMPE_RESAMPLE_OWNERS = 1 };
int pfmpe_get_info(const pfmpe_ctx* ctx, int key, int64_t* value);

/* ----------------------------------------------------------------------- device-resident inputs */
/* Stages a bank of frames' blob lists in HBM (frame f = blobs[offsets[f] .. offsets[f+1]) rows), so a
 * caller replaying recorded detections (or the benchmark) passes bank_frame instead of host pointers. */
int pfmpe_stage_blob_bank(pfmpe_ctx* ctx, const double* blobs, const int32_t* offsets, int nframes);

/* ------------------------------------------------------------------------------ instrumentation */
/* Per-kernel statistics collected while PFMPE_OPT_TIMING is on: launches and summed device time (ms)
 * measured with HIP events on the ctx stream. */
enum { PFMPE_K_PROPAGATE = 0, /* k_propagate_weigh (+ last-block iteration reduce)  */
       PFMPE_K_RESAMPLE = 1,  /* k_resample / k_resample_owners: resampling           */
       PFMPE_K_AUX = 2,       /* hand-off kernels (k_group*, k_top*), regeneration   */
       PFMPE_K_FRAME = 3,     /* k_frame: the whole frame in one launch              */
       PFMPE_K_ROI = 4,       /* k_batch_stage + k_roi_multi* (pfmpe_predict_roi[_multi]) */
       PFMPE_K_FINAL = 5,     /* k_resample_final (non-deferred frames): the record   */
       PFMPE_K_P3P_HIST = 6,  /* k_p3p_hist: initialisation histogram                */
       PFMPE_K_P3P_CHECK = 7, /* k_p3p_check: checkCorrespondences of all candidates */
       PFMPE_K_DETECT = 8,    /* k_det_*: the LED detector pipeline (pfmpe_find_leds) */
       PFMPE_K_COUNT = 9 };
int pfmpe_get_kernel_stats(pfmpe_ctx* ctx, int kernel, int64_t* launches, double* total_ms);
int pfmpe_reset_kernel_stats(pfmpe_ctx* ctx);
const char* pfmpe_kernel_name(int kernel);

/* ------------------------------------------------------------------------------ host-side checks */
/* Pure host functions (no GPU needed): they evaluate the same __host__ __device__ code the kernels use,
 * so CPU tests can pin RNG/geometry semantics against the oracle without a GPU. */
/* j-th (0-based) uniform_real_distribution<double>(a,b) draw of a default_random_engine(seed) */
double pfmpe_host_ref_uniform(uint32_t seed, uint64_t j, double a, double b);
void pfmpe_host_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* twist6 = xi of pose12 about ref_pose12 (the definition at the cloud statistics above), as the kernel forms it */
void pfmpe_host_pose_twist(const double* pose12, const double* ref_pose12, double* twist6);
/* n, M, B, matched and the mode fields of `out` from a votes table (M x (B + 1), row-major; the other fields are
 * zeroed), the function pfmpe_assoc_stats calls after its read-back.  PFMPE_E_ARG for a NULL pointer, M outside
 * 1 .. PFMPE_MAX_MARKERS, B < 0, or rows that do not all sum to the same n. */
int pfmpe_host_assoc_summary(const uint32_t* votes, int M, int B, pfmpe_assoc_out* out);

#ifdef __cplusplus
}
#endif
#endif /* PFMPE_H_ */
