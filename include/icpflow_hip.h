/*
 * icpflow_hip.h -- C ABI of libicpflow_hip.so: the MI355X (gfx950) drop-in for
 * ICP-Flow's cluster-pair registration hot path.
 *
 * Every pointer named d_* is a DEVICE pointer owned by the caller (e.g. the
 * data_ptr() of a torch-ROCm tensor); the library never allocates or frees
 * caller memory and keeps NO mutable process-global state: the only state outside
 * the arguments is a thread-local error string, a thread-local helper stream and
 * per-device caches of immutable device properties.  Tuning switches and the
 * launch-timing recorder travel with each call in an icpflow_options_t.
 * Scratch comes from a caller-provided workspace (icpflow_workspace_bytes()).
 * All work is enqueued asynchronously on `stream` (a hipStream_t passed as
 * void*; NULL = the default stream); no entry point synchronises the device.
 *
 * Return value: 0 = ok, negative = argument error (ICPFLOW_E_*), positive = the
 * hipError_t of a failed runtime call / kernel launch.  icpflow_last_error()
 * returns the message of the calling thread's last failure.  (The reference
 * only printf()s launch errors, hist_cuda_core.cuh:94-98; here they surface.)
 *
 * Data contract (reference: utils_helper.py:185-196 `pad_segment`):
 *   clouds are float32 [B, N, 4] contiguous, columns (x, y, z, flag);
 *   a point is valid iff flag > 0.  The NN / ICP / evaluation entry points
 *   additionally require the layout pad_segment produces -- valid rows first,
 *   then pads -- because, like pytorch3d's `lengths`, they scan the first
 *   n = count(flag > 0) rows.  icpflow_hist_vote accepts arbitrary flag patterns
 *   (the reference's own hist_cuda/test.py uses random flags).
 *   The first n rows of a cloud must be finite: the sorts pad their networks with +inf keys, a NaN
 *   key orders behind that padding, and a sorted row r < n could then name a padding index instead of
 *   a row of the cloud (csrc/sortclouds.hpp, DESIGN.md "The sorts").
 *
 * All citations `file:line` are into the reference repository
 * (yanconglin/ICP-Flow).
 */
#ifndef ICPFLOW_HIP_H
#define ICPFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPFLOW_VERSION 215 /* 0.2.15: icpflow_selftest_peaks_u32 (the peak search on uint32 counters with the fused candidate decode, test only); (icpflow_seq_bucket_table, the cells of the bucket-normalised EPE per class, icpflow_seq_class_table, the per-class and per-speed table of a sample, icpflow_cluster_pcd and icpflow_track_frame_points, cluster_pcd behind the C ABI, icpflow_seq_*, the evaluation of a sequence, icpflow_ego_*, the ego-motion estimate, and icpflow_egomotion_*, its motion compensation and fixed threshold, are additions under the same number: nothing that existed changed; so is ICPFLOW_OPT_NO_FRONT_ROLES, the axis sort and the occupancy grids as workgroups of the vote's launch) 0.2.14: ICPFLOW_OPT_NO_DIR_KEYS (sort keys of the sweeps: horizontal directions next to the axes); 0.2.13: ICPFLOW_OPT_TWO_LAUNCH (ICP of batches of a few rounds: the persistent grid drained for a second launch of whole-CU workgroups; off by default); 0.2.12: ICPFLOW_OPT_NO_SCORE_PREBOUND (scoring sweeps: a scan's whole sum bounded from below by the other cloud's occupancy grid before any target is evaluated); 0.2.11: ICPFLOW_OPT_NO_CHECK_REUSE (hist_icp: the roll-back check takes its sum under the initial pose from the scoring); 0.2.10: ICPFLOW_OPT_NO_VOTE_LIST (the vote's work list on ragged batches); 0.2.9: icpflow_register_stage_begin / _finish, icpflow_associate_frame_begun (stage 2's initial poses beside stage 1's ICP), ICPFLOW_E_HOSTMEM; 0.2.8: ICPFLOW_OPT_NO_SHARED_SCANS (teams: window scans shared by a member's waves); 0.2.7: icpflow_track_frame (one frame pair per call, host half in C++); team-launch chains per device instead of per host thread; 0.2.6: icpflow_register_stage, icpflow_associate_frame (a stage / the rest of match_pcds per call); 0.2.5: options.d_pair_active, icpflow_assoc_assign / _collect (device-side association of a frame pair), ICPFLOW_OPT_TEAMS_HALF_GPU; 0.2.3: icpflow_hist_icp_eval; 0.2.2: icpflow_hist_icp_many; 0.2.1: per-call options replace the process-global switches of 0.1;
                               icpflow_icp takes an initial transform and returns its per-iteration history */

#define ICPFLOW_OK 0
#define ICPFLOW_E_ARG (-1)       /* bad pointer / size / enum                      */
#define ICPFLOW_E_WORKSPACE (-2) /* workspace pointer NULL or too small            */
#define ICPFLOW_E_LIMIT (-3)     /* size beyond what the kernels index (see docs)  */
#define ICPFLOW_E_HOSTMEM (-4)   /* pinned host memory could not be allocated (icpflow_track_frame) */

/* ICP stopping rule */
#define ICPFLOW_STOP_REFERENCE 0 /* batch-global: stop when EVERY pair has rel<=thr
                                    (utils_icp_pytorch3d.py:209); bit-for-bit the
                                    reference's iteration count, no host sync      */
#define ICPFLOW_STOP_PER_PAIR 1  /* each pair stops on its own rel<=thr (or NaN)   */

typedef void *icpflow_stream_t; /* hipStream_t */

int icpflow_version(void);
const char *icpflow_last_error(void);
/* Hash (16 hex digits) of the sources, headers and compiler flags this library was built from
 * (icp_flow_amd/build.py); lets a deployment tell which tree a prebuilt .so belongs to. */
const char *icpflow_build_info(void);

/* ---------------------------------------------------------------------------
 * Per-call options of the fused entry points (last argument; NULL = defaults).
 * Nothing here changes results except icp_arith: every search mode and every
 * ICPFLOW_OPT_* switch selects between implementations that are bit-identical in
 * their outputs (the parity tests run all of them).
 *
 * icp_search -- correspondence search inside the ICP loop:
 *   ICPFLOW_SEARCH_AUTO (0)   sorted sweep when 64 <= N <= 16384, else the all-pairs scan
 *   ICPFLOW_SEARCH_SCAN (1)   all-pairs LDS-tiled scan of the fixed cloud every iteration
 *   ICPFLOW_SEARCH_GRID (2)   exact hashed uniform grid of the fixed cloud, built once per
 *                             registration: only the 27 cells within the gate radius are evaluated
 *   ICPFLOW_SEARCH_SWEEP (3)  both clouds sorted once along the fixed cloud's longest axis; each
 *                             wave scans (LDS broadcast) only the window its queries can gate
 * icp_arith -- arithmetic of the Kabsch step (utils_icp_pytorch3d.py:303-382):
 *   ICPFLOW_ARITH_FP64 (0)    one pass of 18 raw moments in fp64, closed-form rotation in fp64
 *                             (the default: at least as accurate as the reference)
 *   ICPFLOW_ARITH_FP32_REFERENCE (1)  the reference's own operation order in fp32: weighted
 *                             means (:314-315), centring (:318-325), 3x3 product and division
 *                             (:335-336), T = mu_y - mu_x R (:376), rmse from the moved points
 *                             (:191-192) -- reproduces the rounding NOISE LEVEL of the reference's
 *                             tensors (not its bits: the summation order of a GPU reduction differs
 *                             from any other backend's).  All-pairs search, slower; a study mode.
 * profile -- optional recorder of the dominant kernel's launches (see the end of this header).
 * d_vote_bins_u32 -- optional debug output of icpflow_estimate_init_pose / icpflow_hist_icp: the
 *   uint32 bins [B, Lx*Ly*Lz] of the fused (sorted) vote exactly as the peak search reads them.
 * d_icp_init_R [B,3,3], d_icp_init_T [B,3] -- icpflow_icp only, both or neither: `init_transform` of
 *   iterative_closest_point (utils_icp_pytorch3d.py:118-138, scale 1): the first correspondence search runs
 *   on X R0 + T0 instead of X (every iteration still solves for the absolute transform of X).
 * icp_allow_reflection -- icpflow_icp only: `allow_reflection` of corresponding_points_alignment (:354-362): R = U V^T
 *   whatever its determinant (the best ORTHOGONAL matrix; a reflection when det H < 0) instead of the best rotation.
 * icp_estimate_scale, d_icp_scale [B] -- icpflow_icp only: `estimate_scale` of iterative_closest_point (:364-374): the
 *   transform is a similarity, Xt = s X R + T with s = trace(E S) / Xcov; d_icp_scale receives s (may be NULL).
 *   d_icp_init_s [B] (with d_icp_init_R / d_icp_init_T): the scale of the initial transform, NULL = 1.
 * d_icp_history [max_iterations, B, 16] -- icpflow_icp only: `t_history` of the reference's ICPSolution
 *   (:187), i.e. (R row-major 9, T 3, rmse, scale, number of gated correspondences sum(w) of :161, 1 unused) after
 *   every iteration; rows of iterations the batch rule did not reach are unspecified.  Available in the single-launch reference stop mode (max_iterations <= 128,
 *   fp64 arithmetic); otherwise ICPFLOW_E_ARG.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_SEARCH_AUTO 0
#define ICPFLOW_SEARCH_SCAN 1
#define ICPFLOW_SEARCH_GRID 2
#define ICPFLOW_SEARCH_SWEEP 3
#define ICPFLOW_ARITH_FP64 0
#define ICPFLOW_ARITH_FP32_REFERENCE 1
/* developer switches (flags): each turns one optimisation off; results are identical */
#define ICPFLOW_OPT_NO_SORTED_VOTE (1u << 0)  /* all-pairs vote instead of the z-sorted one        */
#define ICPFLOW_OPT_NO_SIDE_STREAM (1u << 1)  /* everything on the caller's stream                 */
#define ICPFLOW_OPT_NO_EVAL_SWEEP (1u << 2)   /* all-pairs match_eval scans                        */
#define ICPFLOW_OPT_NO_CHECK_SWEEP (1u << 3)  /* all-pairs roll-back check                         */
#define ICPFLOW_OPT_NO_SCORE_SWEEP (1u << 4)  /* all-pairs candidate scoring                       */
#define ICPFLOW_OPT_NO_SCORE_PRUNE (1u << 5)  /* every scoring scan runs to the end                */
#define ICPFLOW_OPT_NO_TEAMS (1u << 6)        /* always one workgroup per pair                     */
#define ICPFLOW_OPT_NO_SPECULATIVE (1u << 7)  /* batch-global stop: one launch per iteration       */
#define ICPFLOW_OPT_NO_ADAPTIVE_WINDOWS (1u << 8) /* ICP sweep: no neighbour certificates / probes: every query scans */
#define ICPFLOW_OPT_NO_PERSISTENT (1u << 9)   /* ICP: one workgroup per pair dealt by the hardware dispatcher, whatever B */
#define ICPFLOW_OPT_NO_HELPERS (1u << 10)     /* ICP, persistent grid: workgroups without a pair left do not take passes of others */
/* NOT a bit-identity switch: teams of workgroups (several per large pair) take at most HALF of the CUs, so that two team
 * launches may run side by side (frame pairs in flight; the chains are per device, whatever host threads launch).  The plan -- hence the order of a team's sums --
 * follows the number of workgroups: results equal those of the full-GPU plan to rounding, and are the same whatever else is
 * in flight.  Team launches WITH the flag are chained two deep (two lanes), launches without it wait for both lanes. */
#define ICPFLOW_OPT_TEAMS_HALF_GPU (1u << 11)
/* (a bit-identity switch again) ICP, teams: a wave scans its long windows alone instead of sharing them with the member's other waves */
#define ICPFLOW_OPT_NO_SHARED_SCANS (1u << 12)
/* icpflow_track_frame: stage 2's first half runs behind stage 1 on the caller's stream instead of beside stage 1's ICP on a second
 * one (identical results; the overlap shortens ONE frame pair by ~0.1 ms but registers the whole candidate superset of stage 2 --
 * with several frame pairs in flight on a busy GPU that extra work costs throughput: frame_pairs.register_in_flight sets the flag) */
#define ICPFLOW_OPT_NO_STAGE_OVERLAP (1u << 13)
/* (a bit-identity switch) vote on batches of few wide pairs: the grid covers the padded width of every pair instead of following
 * a work list of the workgroups that have rows, largest pairs first */
#define ICPFLOW_OPT_NO_VOTE_LIST (1u << 14)
/* (a bit-identity switch) icpflow_hist_icp and the entry points built on it: the roll-back check (utils_icp.py:27-35) scans under the
 * initial pose as well, instead of taking that sum from the candidate scoring, whose forward scan of the picked candidate
 * (utils_hist.py:86-101) is the same scan of the same points */
#define ICPFLOW_OPT_NO_CHECK_REUSE (1u << 15)
/* (a bit-identity switch) candidate scoring as pruned sweeps: no occupancy grids of the sorted clouds, i.e. a scan is only ever
 * ended by the lower bounds its waves accumulate while they evaluate targets */
#define ICPFLOW_OPT_NO_SCORE_PREBOUND (1u << 16)
/* (a bit-identity switch, OFF by default: it does not pay -- DESIGN.md 8) ICP of a batch of two to four rounds of half-CU workgroups
 * under the reference's batch-global stop (utils_icp_pytorch3d.py:153-213): the persistent grid is DRAINED once the unfinished pairs
 * fit one CU each (they leave behind their current iteration, still moving), and a second launch gives each of them a 1024-thread
 * workgroup and resumes it at its own iteration from its history rows (icp_epilogue.hip: icp_split_kernel).  Same sums (added in the order of
 * the 64-query units in either kernel), same history: transforms and iteration counts are those of one launch, bit for bit. */
#define ICPFLOW_OPT_TWO_LAUNCH (1u << 17)
/* (NOT strictly a bit-identity switch: same neighbours, gate decisions, iteration counts and picks; the queries of a pair are visited in
 * another order, so its fp64 moment sums are added in another order -- measured: 1 transform in 8192 differs in one bit, 1.5e-13 m)
 * the sorted sweeps (ICP search, candidate scoring, roll-back check, match_eval): both clouds of every pair are
 * sorted along the fixed cloud's longest AXIS, as before round 6, instead of by the key -- an axis or one of six horizontal
 * directions -- that spreads the fixed cloud best (a vehicle heading along an axis shows a face across it: a third of its points on
 * one key).  The searches are exact under any such key: same neighbours, same sums (utils_icp_pytorch3d.py:153-168, utils_hist.py:86-101) */
#define ICPFLOW_OPT_NO_DIR_KEYS (1u << 18)
/* (a bit-identity switch) icpflow_hist_icp and the entry points built on it: the axis sort of both clouds and the occupancy grids
 * run beside the vote on a second stream, forked from and joined into the caller's, instead of as workgroups of the vote's own
 * launch, in front of the vote's (batches of up to 4096 points per cloud whose vote gives four waves to every 64 rows) */
#define ICPFLOW_OPT_NO_FRONT_ROLES (1u << 19)

typedef struct icpflow_profile icpflow_profile_t; /* opaque */

typedef struct icpflow_options {
    size_t struct_size; /* sizeof(icpflow_options_t) of the caller's header */
    int icp_search;
    int icp_arith;
    unsigned flags;
    icpflow_profile_t *profile;
    uint32_t *d_vote_bins_u32;
    const float *d_icp_init_R;
    const float *d_icp_init_T;
    float *d_icp_history;
    int icp_allow_reflection;
    int icp_estimate_scale;
    float *d_icp_scale;
    const float *d_icp_init_s;
    /* icpflow_hist_icp / icpflow_hist_icp_eval: uint8 [B] or NULL.  Pairs flagged 0 are NOT IN THE BATCH: the batch-global
     * stop of the ICP (utils_icp_pytorch3d.py:209) is taken over the flagged pairs only, their outputs are unspecified.  For
     * callers that must size a batch before the device has decided which of its candidate pairs exist (stage 2 of match_pcds
     * enqueued before stage 1's results are known: icpflow_assoc_assign); the caller hands such pairs over as EMPTY clouds
     * (all flags 0), so that every other kernel of the path skips them.  Reference stop rule, max_iterations <= 128 only. */
    const uint8_t *d_pair_active;
} icpflow_options_t;

/* Bytes of device scratch the fused entry points below need for a batch of B
 * pairs padded to N points with a translation histogram of Lx*Ly*Lz bins.
 * (Pass Lx=Ly=Lz=0 for entry points that do not vote.) */
size_t icpflow_workspace_bytes(int B, int N, int Lx, int Ly, int Lz);

/* ---------------------------------------------------------------------------
 * a-1  translation-histogram vote.
 * Replaces: HIST.hist / hist_cuda() -- hist_cuda/hist.py:39-51, cpp/hist.cpp:4-27,
 * cpp/hist_cuda.cu:19-90, kernel cpp/hist_cuda_core.cuh:23-64.
 * For every valid i in X[b], valid j in Y[b]: v = X_i - Y_j; if min <= v < max on
 * all axes, p = floor((v-min)/(max-min)*float(len)) and bins[b,px,py,pz] += 1.
 * d_bins: float32 [B, len_x, len_y, len_z], fully overwritten (the reference
 * returns a fresh zero-initialised tensor, hist_cuda.cu:59).  Bit-exact with the
 * reference's integer-valued float counters; `mini_batch` of the reference only
 * chunks launches (hist_cuda.cu:61-85) and has no equivalent here.
 * ------------------------------------------------------------------------- */
int icpflow_hist_vote(const float *d_X, const float *d_Y, int B, int NX, int NY,
                      float min_x, float min_y, float min_z,
                      float max_x, float max_y, float max_z,
                      int len_x, int len_y, int len_z,
                      float *d_bins, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-2  3-D non-maximum suppression + top-k peaks.
 * Replaces: topk_nms -- utils_hist.py:21-29 (max_pool3d(kernel, stride 1,
 * pad (kernel-1)/2) == x, then topk over the flattened surviving votes).
 * d_votes float32 [B,k], d_idx int64 [B,k] (flat index into [Lx,Ly,Lz]).
 * Order: vote descending, ties by ascending flat index (torch.topk's order among
 * equal votes is implementation-defined; this rule is deterministic).
 * The bins are vote counts, i.e. non-negative integers, read as uint32_t (the vote returned is float32 of that integer).
 * d_ws: at least 2 * (B*Lx*Ly*Lz * 4 rounded up to a multiple of 256) bytes of scratch.
 * ------------------------------------------------------------------------- */
int icpflow_hist_peaks(const float *d_bins, int B, int len_x, int len_y, int len_z,
                       int k, int kernel_size, float *d_votes, int64_t *d_idx,
                       void *d_ws, size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-4  brute-force K=1 nearest neighbour, both clouds scanned in full.
 * Replaces: nearest_neighbor_batch -- utils_helper.py:20-30, i.e.
 * pytorch3d.ops.knn_points(src[:,:,0:3], dst[:,:,0:3], K=1) followed by sqrt.
 * d_Q float32 [B,NQ,q_stride], d_T float32 [B,NT,t_stride] (strides in floats,
 * >= 3; the first three columns are x,y,z).  d_len_q / d_len_t: optional int32
 * [B] valid prefixes (pytorch3d `lengths1/2`, utils_icp_pytorch3d.py:154-156);
 * NULL = all NQ / NT rows, pads included, exactly like the reference's
 * un-lengthed call.  Rows >= len_q get idx 0 / dist 0 (pytorch3d convention).
 * d_idx int64 [B,NQ]; d_dist float32 [B,NQ]: Euclidean distance if
 * sqrt_dist != 0, squared distance otherwise.  First minimum wins ties.
 * ------------------------------------------------------------------------- */
int icpflow_nn_batch(const float *d_Q, const float *d_T, int B, int NQ, int NT,
                     int q_stride, int t_stride, const int32_t *d_len_q,
                     const int32_t *d_len_t, int sqrt_dist, int64_t *d_idx,
                     float *d_dist, icpflow_stream_t stream);

/* a-10  transform_points_batch -- utils_helper.py:76-87:
 * out[b,i,0:3] = [x y z 1] * pose[b]^T, flag column copied.  In-place allowed. */
int icpflow_transform_points(const float *d_xyz, const float *d_pose, int B, int N,
                             float *d_out, icpflow_stream_t stream);

/* Number of valid points per pair: d_len[b] = count(flag > 0) (int32 [B]). */
int icpflow_count_valid(const float *d_pts, int B, int N, int32_t *d_len,
                        icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * a-3  initial pose from the translation histogram.
 * Replaces: estimate_init_pose / estimate_init_pose_batch -- utils_hist.py:33-124
 * (vote with X=dst, Y=src; NMS + top-5; decode to left bin edges; append the zero
 * translation; score the 6 candidates by min(mean fwd NN dist, mean bwd NN dist)
 * over valid points; first arg-min).  `chunk_size` of the reference only bounds
 * memory and does not change results, so it has no equivalent.
 * d_edges_{x,y,z}: float32 left bin edges exactly as the reference builds them
 * (torch.arange, utils_hist.py:63-65); vote box = [edges[0], edges[L-1]) with L bins
 * (the reference passes bins.min()/bins.max()/len(bins), utils_hist.py:69-72).
 * decode_shift = thres_dist // 2 (utils_hist.py:78; 0.0 for thres_dist 0.1).
 * d_T_out float32 [B,4,4]: identity with the winning translation in column 3.
 * ------------------------------------------------------------------------- */
int icpflow_estimate_init_pose(const float *d_src, const float *d_dst, int B, int N,
                               const float *d_edges_x, int len_x,
                               const float *d_edges_y, int len_y,
                               const float *d_edges_z, int len_z,
                               float decode_shift, float *d_T_out,
                               void *d_ws, size_t ws_bytes, icpflow_stream_t stream,
                               const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-5..a-7  masked batched point-to-point ICP.
 * Replaces: iterative_closest_point -- utils_icp_pytorch3d.py:37-225 with
 * corresponding_points_alignment (:233-382) and _apply_similarity_transform
 * (:385-396), estimate_scale=False, allow_reflection=False.
 * Per iteration: NN of the current X in Y (valid prefixes), gate d^2 <= thres^2,
 * Kabsch on the gated pairs FROM THE ORIGINAL X (absolute, not incremental),
 * rmse, relative-rmse stop (see ICPFLOW_STOP_*).  Row-vector convention
 * y = x R + T as in the reference.
 * d_pre_pose: optional float32 [B,4,4]; when non-NULL the ICP input is
 * transform_points_batch(X, pre_pose) (utils_icp.py:21) computed on the fly.
 * Thresholds are passed as the reference's Python doubles and narrowed exactly where
 * torch narrows them: the gate compares the fp32 squared distance with
 * (float)(thres*thres) (= 0x3C23D70A for 0.1; squaring the fp32 value 0.1f instead would
 * give the next float up), the stop compares with (float)relative_rmse_thr.
 * Outputs (any may be NULL): d_R [B,3,3], d_T [B,3], d_rmse [B],
 * d_iters int32 [1] (loop bodies executed; per-pair mode: max over pairs),
 * d_converged int32 [1].
 * Failure inside the launch: when several workgroups share one large pair (N > 1024, batch smaller
 * than half the GPU) and a member is not scheduled for 2 s -- another process saturating the GPU --
 * the registration is abandoned instead of hanging the queue: every R of the batch is NaN and
 * *d_iters = -1 (also for icpflow_apply_icp / icpflow_hist_icp, whose transforms are then NaN).
 * Callers must treat iters < 0 as an error (the Python mirrors raise).
 * ------------------------------------------------------------------------- */
int icpflow_icp(const float *d_X, const float *d_Y, const float *d_pre_pose, int B, int N,
                double thres, int max_iterations, double relative_rmse_thr, int stop_mode,
                float *d_R, float *d_T, float *d_rmse, int32_t *d_iters,
                int32_t *d_converged, void *d_ws, size_t ws_bytes,
                icpflow_stream_t stream, const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-8, a-9  ICP from an initial pose with roll-back.
 * Replaces: apply_icp + pytorch3d_icp -- utils_icp.py:20-73 (pre-transform src,
 * ICP with max_iterations / relative_rmse_thr (reference: 100 / 1e-6), 4x4 =
 * [[R^T, T],[0,0,0,1]] * init, mean NN error of valid src before / after, and
 * `Rts[error_icp >= error_init] = init`).
 * d_T_out float32 [B,4,4]; may alias d_init.
 * ------------------------------------------------------------------------- */
int icpflow_apply_icp(const float *d_src, const float *d_dst, const float *d_init,
                      int B, int N, double thres_dist, int max_iterations,
                      double relative_rmse_thr, int stop_mode, float *d_T_out,
                      int32_t *d_iters, void *d_ws, size_t ws_bytes,
                      icpflow_stream_t stream, const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-11  one full registration per cluster pair.
 * Replaces: hist_icp -- utils_match.py:138-157 (register the cloud with fewer
 * valid points onto the other (strict >, ties not swapped), a-3 then a-9, and
 * invert the 4x4 of swapped pairs).  The swap is done by pointer selection, the
 * inputs are never copied.  The inverse is the analytic rigid inverse (the
 * reference's general torch.linalg.inv leaves ~1e-8 noise in the bottom row).
 * d_T_out float32 [B,4,4] maps the ORIGINAL src onto dst.
 * ------------------------------------------------------------------------- */
int icpflow_hist_icp(const float *d_src, const float *d_dst, int B, int N,
                     const float *d_edges_x, int len_x,
                     const float *d_edges_y, int len_y,
                     const float *d_edges_z, int len_z,
                     float decode_shift, double thres_dist, int max_iterations,
                     double relative_rmse_thr, int stop_mode, float *d_T_out,
                     int32_t *d_iters, void *d_ws, size_t ws_bytes,
                     icpflow_stream_t stream, const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-11, several batches in flight.  K independent calls of icpflow_hist_icp (same N, histogram and ICP parameters;
 * batch k: d_src[k], d_dst[k] of B[k] pairs, outputs d_T_out[k], d_iters[k], its OWN workspace d_ws[k] of
 * ws_bytes[k] >= icpflow_workspace_bytes(B[k], N, ...)), enqueued on internal worker streams that are forked from and
 * joined back into `stream`: to the caller it is one asynchronous call on `stream`.  Every batch keeps its own
 * batch-global ICP stop (utils_icp_pytorch3d.py:209 couples the pairs of ONE hist_icp call, utils_match.py:138-157) and
 * its results are bit-identical to a call of its own; what the overlap buys is the tail of one batch's ICP launch
 * -- few pairs still iterating, most CUs idle -- running under the vote and scoring of the others.  The reference
 * has no counterpart (it registers one batch after the other, main.py:184-215); frame pairs and association stages
 * of different frames are independent and can be registered this way.
 * ------------------------------------------------------------------------- */
int icpflow_hist_icp_many(int K, const float *const *d_src, const float *const *d_dst, const int *B, int N,
                          const float *d_edges_x, int len_x, const float *d_edges_y, int len_y,
                          const float *d_edges_z, int len_z, float decode_shift, double thres_dist,
                          int max_iterations, double relative_rmse_thr, int stop_mode, float *const *d_T_out,
                          int32_t *const *d_iters, void *const *d_ws, const size_t *ws_bytes,
                          icpflow_stream_t stream, const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-12  registration quality metrics.
 * Replaces: match_eval -- utils_match.py:159-213.  All outputs float32:
 * d_errors, d_inliers, d_ratios, d_ious [B,2] (src direction, dst direction);
 * d_translations [B,3]; d_rotations [B,3] (Euler ZYX, degrees).
 * ------------------------------------------------------------------------- */
int icpflow_match_eval(const float *d_pcd1, const float *d_pcd2, const float *d_T,
                       int B, int N, double thres_dist, float *d_errors,
                       float *d_inliers, float *d_ratios, float *d_ious,
                       float *d_translations, float *d_rotations, void *d_ws,
                       size_t ws_bytes, icpflow_stream_t stream, const icpflow_options_t *opt);

/* a-11 + a-12 in one call: icpflow_hist_icp followed by icpflow_match_eval of the same clouds under the transforms it
 * found (utils_match.py:92-93: `hist_icp(...)` then `match_eval(...)`, every candidate pair of match_pairs).  Same
 * results as the two calls; the metrics reuse what the registration left in the workspace (valid-row counts, both clouds
 * sorted along one axis) instead of counting and sorting again.  Arguments as in the two entry points. */
int icpflow_hist_icp_eval(const float *d_src, const float *d_dst, int B, int N, const float *d_edges_x, int len_x,
                          const float *d_edges_y, int len_y, const float *d_edges_z, int len_z, float decode_shift,
                          double thres_dist, int max_iterations, double relative_rmse_thr, int stop_mode,
                          float *d_T_out, int32_t *d_iters, float *d_errors, float *d_inliers, float *d_ratios,
                          float *d_ious, float *d_translations, float *d_rotations, void *d_ws, size_t ws_bytes,
                          icpflow_stream_t stream, const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * a-15 / 8(f)  helpers of the host association around the path.
 *
 * icpflow_gather_pad builds the padded batch of match_pairs (utils_match.py:81-91 with
 * pad_segment, utils_helper.py:185-196): d_rows int32 [B,N] holds, per pair and slot, the row of
 * d_points ([M,3] float32) to copy (flag 1) or -1 for a pad row (1e8,1e8,1e8,0).  The caller
 * decides the rows (cluster order, random subsample of over-long clusters).
 *
 * icpflow_gather_segments builds the same batch straight from the label-sorted row table d_order
 * (int64 [M]): d_seg int64 [3,B] holds per pair the first row of its cluster in d_order, the number of
 * rows to take (<= N) and -1 or an offset into d_perm (int32) when the host subsampled an over-long
 * cluster (random_choice, utils_helper.py:198-201): row i = d_order[start + d_perm[off + i]].
 *
 * icpflow_cluster_stats reduces what sanity_check reads per cluster (utils_check.py:34-43,
 * get_bbox_tensor utils_helper.py:166-170): d_order int64 [M] = rows of d_points ([M,3]) sorted by
 * label, cluster c = d_order[d_start[c] .. d_start[c]+d_count[c]) (int64 [L] each); outputs the
 * centroid d_mean [L,3] and the ascending-sorted bbox extents d_extent [L,3] (float32).  d_labels
 * (float32 [L], optional): clusters with a negative label (ground, noise -- never candidates,
 * utils_check.py:32) are skipped and report zeros.
 *
 * icpflow_flow_rigid replaces flow_estimation_torch (utils_flow.py:57-69): every point whose
 * float label equals d_pair_labels[p] moves with T[p]*pose, every other point with pose alone;
 * flow = moved - point.  d_ws: not used since version 204 (may be NULL).
 * ------------------------------------------------------------------------- */
int icpflow_gather_pad(const float *d_points, const int32_t *d_rows, int B, int N, float *d_out,
                       icpflow_stream_t stream);
/* Device-side association of a frame pair (match_pairs' host half, utils_match.py:96-115, as kernels -- so that match_pcds can
 * enqueue both of its stages and the flow without reading a stage's results back).
 *
 * icpflow_assoc_assign: one association stage.  d_result = the results of icpflow_hist_icp_eval for the stage's K candidate
 * pairs, float32 array after array [T 16K | errors 2K | inliers 2K | ratios 2K | ious 2K | translations 3K | rotations 3K];
 * candidate k pairs source cluster d_si[k] (row of the source table, < S) with destination cluster d_di[k] (< D); d_active
 * (uint8 [K] or NULL): candidates flagged 0 do not exist.  A candidate survives check_transformation (utils_check.py:51-66)
 * iff |translation| <= translation_frame, min(iou) >= thres_iou and max(|rot_y|, |rot_x|) <= rot_limit_deg; every source
 * row takes the surviving candidate with the smallest min(error_src, error_dst), ties to the smallest destination row
 * (np.argmin's first minimum, utils_helper.py:108-110), if that error is < thres_error (utils_match.py:112): d_best int32 [S]
 * receives its index or -1.  With K2 > 0 the NEXT stage's candidates (d_si2, d_di2 [K2]) are switched on or off in the same
 * launch (utils_match.py:45-53: only clusters that found no partner go on): d_active2 uint8 [K2], and the lengths of the
 * inactive ones in d_seg2 (int64 [2,3,K2], the segment rows of icpflow_gather_segments for both clouds) are set to 0.
 *
 * icpflow_assoc_collect: the pair rows of both stages, stage 1 first, each in ascending source row: d_rows float32 [cap,10]
 * (source label, destination label, errors, inliers, ratios, ious: utils_match.py:120-131), d_T float32 [cap,16]; rows beyond
 * the matches carry the label -3e38 (no point has it) and the identity.  d_count int32: the number of matches written, at most
 * `cap` (matches beyond the first `cap`, in that order, are dropped), or -1 when a stage reported an abandoned batch
 * (iteration count < 0).  Labels: float64 tables with `label_stride` doubles per row (the d_table of icpflow_cluster_table).
 * Stage 2 may be absent (K2 = 0). */
int icpflow_assoc_assign(const float *d_result, const int32_t *d_si, const int32_t *d_di, int K, const uint8_t *d_active,
                         int S, int D, float translation_frame, float thres_iou, float rot_limit_deg, float thres_error,
                         int32_t *d_best, int K2, const int32_t *d_si2, const int32_t *d_di2, int64_t *d_seg2,
                         uint8_t *d_active2, icpflow_stream_t stream);
int icpflow_assoc_collect(const int32_t *d_best1, const float *d_result1, const int32_t *d_si1, const int32_t *d_di1, int K1,
                          const int32_t *d_best2, const float *d_result2, const int32_t *d_si2, const int32_t *d_di2, int K2,
                          const double *d_src_table, const double *d_dst_table, int label_stride, int S, int cap,
                          float *d_rows, float *d_T, int32_t *d_count, icpflow_stream_t stream);
int icpflow_gather_segments(const float *d_points, const int64_t *d_order, const int64_t *d_seg,
                            const int32_t *d_perm, int B, int N, float *d_out, icpflow_stream_t stream);

/* The same, one call per stage instead of one per kernel (version 206) -- match_pairs (utils_match.py:69-136) and match_pcds
 * (utils_match.py:26-66) from the cluster tables on.  A frame pair in flight costs its host thread a fixed price per call
 * into the library; these two take what used to be ten.
 *
 * icpflow_tables_t: both clouds of the frame pair as icpflow_cluster_table leaves them (points float32 rows of 3, the
 * label-sorted order, the float64 table with `label_stride` doubles per cluster, label first; S and D clusters).
 * icpflow_stage_t: K candidate pairs of an association stage.  d_seg int64 [2,3,K] are the segment rows of
 * icpflow_gather_segments (start, length, offset of the subsample in d_perm or -1; source cloud first), d_si / d_di int32 [K]
 * the table rows of each candidate, N the width of the padded batch; d_clouds float32 [2,K,N,4] is scratch for the padded
 * batch, d_result float32 [30 K + 1] receives the results of icpflow_hist_icp_eval, array after array
 * [T 16K | errors 2K | inliers 2K | ratios 2K | ious 2K | translations 3K | rotations 3K | iteration count (int32)].
 * icpflow_registration_t: the arguments of icpflow_hist_icp_eval that do not depend on the batch.
 *
 * icpflow_register_stage: pad_segment of both clouds (utils_match.py:81-91) + hist_icp + match_eval of one stage.
 * icpflow_associate_frame: everything of match_pcds behind stage 1's registration (`stage1`, registered by
 *   icpflow_register_stage on the same stream): icpflow_assoc_assign of stage 1 (which switches stage 2's candidates on or
 *   off: d_active2 uint8 [stage2->K], scratch), icpflow_register_stage of stage 2 with options.d_pair_active = d_active2,
 *   icpflow_assoc_assign of stage 2, icpflow_assoc_collect (d_best int32 [2 S + 2]: stage 1's choice per source row, stage
 *   2's, the number of matches; d_rows [cap,10], d_T [cap,16]) and, with d_flow != NULL, icpflow_flow_rigid_rows of n_flow
 *   points on the padded pair rows.  stage2 may be NULL or have K = 0.  d_ws / ws_bytes: icpflow_workspace_bytes of the
 *   larger stage. */
typedef struct icpflow_tables {
    const float *d_points_src;
    const int64_t *d_order_src;
    const double *d_table_src;
    const float *d_points_dst;
    const int64_t *d_order_dst;
    const double *d_table_dst;
    int S, D, label_stride;
} icpflow_tables_t;

typedef struct icpflow_stage {
    const int64_t *d_seg;
    const int32_t *d_perm;
    const int32_t *d_si;
    const int32_t *d_di;
    float *d_clouds;
    float *d_result;
    int K, N;
} icpflow_stage_t;

typedef struct icpflow_registration {
    const float *d_edges_x;
    const float *d_edges_y;
    const float *d_edges_z;
    int len_x, len_y, len_z;
    float decode_shift;
    double thres_dist;
    double relative_rmse_thr;
    int max_iterations;
    int stop_mode;
} icpflow_registration_t;

int icpflow_register_stage(const icpflow_tables_t *tables, const icpflow_stage_t *stage, const icpflow_registration_t *reg,
                           void *d_ws, size_t ws_bytes, icpflow_stream_t stream, const icpflow_options_t *opt);
int icpflow_associate_frame(const icpflow_tables_t *tables, const icpflow_stage_t *stage1, const icpflow_stage_t *stage2,
                            uint8_t *d_active2, const icpflow_registration_t *reg, float translation_frame, float thres_iou,
                            float rot_limit_deg, float thres_error, int32_t *d_best, int cap, float *d_rows, float *d_T,
                            const float *d_flow_points, const float *d_flow_labels, int n_flow, const float *d_pose,
                            float *d_flow, void *d_ws, size_t ws_bytes, icpflow_stream_t stream,
                            const icpflow_options_t *opt);
/* (version 209) icpflow_register_stage in two halves, so that a frame pair's stage 2 can estimate its initial poses on another
 * stream BESIDE stage 1's ICP (a chain of dependent iterations on a few long pairs that leaves most of the GPU idle):
 * _begin gathers the clouds of the WHOLE candidate list and enqueues lengths, sorts, vote, peaks and scoring (utils_hist.py:82-124)
 * -- and, where one speculative launch runs the batch rule (reference stop, 2 <= max_iterations <= 128, fp64 arithmetic), the ICP of
 * ALL candidates (h_carry[2] = 1) -- on `stream`, leaving initial poses (and trajectories) in d_ws and a few host words in h_carry;
 * _finish enqueues the rest (the batch rule over the pairs that are in the batch after all, found from the trajectories; else the ICP
 * itself; roll-back check, metrics; utils_icp.py:20-35, utils_match.py:159-213) from that workspace -- options.d_pair_active of the second call says which
 * candidates are in the batch after all: the others keep their clouds and are passed over by every kernel (their result rows are
 * unspecified).  The pairs in the batch get bit for bit what icpflow_register_stage gives them with the others handed over as
 * empty clouds.  The caller orders the two calls (an event from _begin's stream to _finish's); d_ws must not be used in between.
 * icpflow_associate_frame_begun: icpflow_associate_frame for a stage 2 that has been begun (d_ws2 / h_carry2: its workspace). */
int icpflow_register_stage_begin(const icpflow_tables_t *tables, const icpflow_stage_t *stage, const icpflow_registration_t *reg,
                                 void *d_ws, size_t ws_bytes, icpflow_stream_t stream, const icpflow_options_t *opt,
                                 int32_t *h_carry /* [4] */);
int icpflow_register_stage_finish(const icpflow_tables_t *tables, const icpflow_stage_t *stage, const icpflow_registration_t *reg,
                                  void *d_ws, size_t ws_bytes, icpflow_stream_t stream, const icpflow_options_t *opt,
                                  const int32_t *h_carry /* [4] */);
int icpflow_associate_frame_begun(const icpflow_tables_t *tables, const icpflow_stage_t *stage1, const icpflow_stage_t *stage2,
                                  uint8_t *d_active2, const icpflow_registration_t *reg, float translation_frame, float thres_iou,
                                  float rot_limit_deg, float thres_error, int32_t *d_best, int cap, float *d_rows, float *d_T,
                                  const float *d_flow_points, const float *d_flow_labels, int n_flow, const float *d_pose,
                                  float *d_flow, void *d_ws2, size_t ws2_bytes, icpflow_stream_t stream,
                                  const icpflow_options_t *opt, const int32_t *h_carry2 /* [4] */);
/* ---------------------------------------------------------------------------
 * One frame pair per call (version 207): match_pcds (utils_match.py:24-66) + flow_estimation_torch (utils_flow.py:57-69) from two
 * labelled clouds on, the HOST half included -- cluster tables, candidate lists, sanity_check (utils_check.py:21-49), padded
 * batches with the reference's stream of random subsamples, both association stages (device-side association: icpflow_
 * register_stage + icpflow_associate_frame), the flow.  BLOCKING: returns when the results are complete on the device (two
 * waits inside: the cluster tables, the end).  A host thread per frame pair in flight, each on its own stream, keeps several
 * going: the time a Python host spends between the calls of the finer-grained entry points is what binds a stream of frame
 * pairs.
 *
 * d_points_* float32 [n,3], d_labels_* float32 [n].  par: the flags of the reference's argument parser that the path reads
 * (main.py / demo.sh) + `seed`: the over-long clusters of stage 1 are subsampled by torch.randperm's algorithm on MT19937
 * seeded with it (= torch.Generator().manual_seed(seed), the generator frame_pairs.py gives every frame pair).
 * Outputs: d_rows float32 [1024,10], d_T float32 [1024,16] (the first *h_pairs rows are the matches, the rest padding),
 * d_flow float32 [n_src,3] of d_flow_points (or NULL: no flow) under d_pose [4,4].  *h_pairs: the number of matched pairs;
 * ICPFLOW_FRAME_HOST_PATH when this call cannot serve the frame pair (no candidate pair at all, more than 512 clusters: the caller runs
 * the finer-grained path, nothing was consumed).  When a stage-2 candidate with a cluster too long for the superset turns out
 * to be needed, the call registers stage 2 once more the reference's way -- its exact candidates, read from stage 1's
 * assignment, subsamples drawn next from the same generator -- on top of stage 1's results (one more wait); ICPFLOW_FRAME_ABANDONED when a team's wait timed out (transforms NaN).  d_scratch / scratch_bytes: device
 * scratch; on ICPFLOW_E_WORKSPACE *scratch_needed says how much this frame pair needs (call again with that much).
 * ------------------------------------------------------------------------- */
#define ICPFLOW_FRAME_HOST_PATH (-2)
#define ICPFLOW_FRAME_HOST_ASSOCIATION (-3) /* (reserved: as HOST_PATH, and the device-side association cannot serve the frame pair either) */
#define ICPFLOW_FRAME_ABANDONED (-1)
/* The state of torch's CPU generator (at::mt19937): the 624 words and how many of them have been consumed (624 = the next
 * draw regenerates the block; a generator fresh from manual_seed).  icp_flow_amd/_lib.py converts to and from
 * torch.Generator.get_state(). */
typedef struct icpflow_mt19937 {
    uint32_t state[624];
    int32_t index;
} icpflow_mt19937_t;
typedef struct icpflow_frame_params {
    size_t struct_size;       /* sizeof(icpflow_frame_params_t) */
    uint64_t seed;            /* the draws start from torch.Generator().manual_seed(seed) ... */
    icpflow_mt19937_t *generator; /* ... or, when not NULL, from this state, which is advanced (only when the call serves the frame pair) */
    int max_points;           /* --max_points */
    int min_cluster_size;     /* --min_cluster_size */
    float translation_frame;  /* --translation_frame (or 2 * speed * gap, main.py:200) */
    float thres_box;          /* --thres_box */
    float thres_iou;          /* --thres_iou */
    float rot_limit_deg;      /* --thres_rot * 90 */
    float thres_error;        /* --thres_error */
    int tight_padding;        /* 1: batches as wide as their longest cluster (icp_flow_amd's default), 0: max_points wide */
    int superset_width;       /* clusters above it stay out of stage 2's superset (0 = 1024) */
} icpflow_frame_params_t;
int icpflow_track_frame(const float *d_points_src, const float *d_labels_src, int n_src, const float *d_points_dst,
                        const float *d_labels_dst, int n_dst, const icpflow_registration_t *reg,
                        const icpflow_frame_params_t *par, float *d_rows, float *d_T, int32_t *h_pairs,
                        const float *d_flow_points, const float *d_pose, float *d_flow, void *d_scratch,
                        size_t scratch_bytes, size_t *scratch_needed, icpflow_stream_t stream,
                        const icpflow_options_t *opt);
/* torch.randperm(n, generator)[0:take] as this library restates it (host only; the CPU tests pin it against torch) */
int icpflow_selftest_randperm(icpflow_mt19937_t *gen, int64_t n, int take, int32_t *h_out);

int icpflow_cluster_stats(const float *d_points, const int64_t *d_order, const int64_t *d_start,
                          const int64_t *d_count, const float *d_labels, int L, float *d_mean,
                          float *d_extent, icpflow_stream_t stream);
/* icpflow_cluster_table: everything match_pcds needs to know about the clusters of ONE labelled cloud, in one chain of
 * launches: d_order int64 [M] = the rows sorted by label, STABLE (rows of a cluster in their original order: the
 * reference's random subsample of over-long clusters, utils_helper.py:198-201, indexes into that order); d_table
 * float64 [Lmax, 9], row c = (label, number of rows, first position in d_order, centroid x y z, bounding-box extents in
 * ascending order) of the c-th distinct label in ascending order -- what torch.unique(labels) (utils_match.py:27-29),
 * the per-pair masks (:81-86) and sanity_check (utils_check.py:34-43, get_bbox_tensor utils_helper.py:166-170) compute
 * cluster by cluster; centroid and extents are zero for negative labels (ground, noise: never candidates,
 * utils_check.py:32).  d_num int32 [1]: the number of distinct labels, or its negative when it exceeds Lmax (<= 4096;
 * the table then holds nothing usable).  float64 carries the float32 statistics and the counts exactly.  -0.0 and +0.0
 * are one label, reported as 0.0 (as torch.unique and every `==` on labels see them); NaN labels are one cluster per bit
 * pattern, positive NaNs after +inf and negative NaNs before -inf, with statistics. */
size_t icpflow_cluster_table_workspace_bytes(int M, int Lmax);
int icpflow_cluster_table(const float *d_points, const float *d_labels, int M, int64_t *d_order, double *d_table, int Lmax,
                          int32_t *d_num, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);
/* The tables of BOTH clouds of a frame pair (what match_pcds needs before anything else, utils_match.py:27-29) in one
 * chain of launches -- half as many as two icpflow_cluster_table calls; every output exactly what those calls write. */
size_t icpflow_cluster_table_pair_workspace_bytes(int MA, int MB, int Lmax);
int icpflow_cluster_table_pair(const float *d_points_a, const float *d_labels_a, int MA, int64_t *d_order_a,
                               double *d_table_a, int32_t *d_num_a, const float *d_points_b, const float *d_labels_b,
                               int MB, int64_t *d_order_b, double *d_table_b, int32_t *d_num_b, int Lmax, void *d_ws,
                               size_t ws_bytes, icpflow_stream_t stream);
int icpflow_flow_rigid(const float *d_points, const float *d_labels, int N, const float *d_pair_labels,
                       const float *d_T, int P, const float *d_pose, float *d_flow, void *d_ws,
                       size_t ws_bytes, icpflow_stream_t stream);
/* The same with the matched source labels read where match_pcds leaves them: column 0 of its pair rows (d_pair_rows
 * float32 [P, pair_stride], pair_stride = 10 for the [P,10] rows of utils_match.py:118-127; 1 = a plain array). */
int icpflow_flow_rigid_rows(const float *d_points, const float *d_labels, int N, const float *d_pair_rows,
                            int pair_stride, const float *d_T, int P, const float *d_pose, float *d_flow,
                            icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(f) row 4  density clustering of a frame pair's points -- the `cluster_dbscan` branch of
 * cluster_pcd (utils_cluster.py:32-48, 50-63), i.e. open3d 0.17.0 PointCloud::cluster_dbscan(eps,
 * min_points) (environment.yml:227; third-party, not in the reference tree).
 *
 * d_points float32 rows of `stride` floats (x, y, z first), n rows.  d_mask (uint8 [n], optional):
 * rows with mask 0 are not clustered (the ground rows of cluster_pcd's idxs_nonground) and report -2.
 * A neighbour is a point whose squared distance, evaluated in fp64, is STRICTLY below eps^2; a point
 * with >= min_points neighbours (itself included) is a core point.
 * Outputs: d_labels int32 [n]: cluster id 0..C-1 in order of each cluster's smallest core-point row
 * (Open3D's numbering), -1 noise, -2 masked out;  d_counts int32 [n]: the first C entries are the
 * cluster sizes;  d_num_clusters int32 [1] = C.  Keeping only the num_clusters largest clusters
 * (utils_cluster.py:38-45) is not part of this call: icpflow_cluster_pcd below does it on the device (its keep-rule
 * kernel reads d_counts); icp_flow_amd/utils_cluster.py's default path still does it in numpy.
 * ------------------------------------------------------------------------- */
size_t icpflow_dbscan_workspace_bytes(int n);
int icpflow_dbscan(const float *d_points, int stride, const uint8_t *d_mask, int n, double eps, int min_points,
                   int32_t *d_labels, int32_t *d_counts, int32_t *d_num_clusters, void *d_ws, size_t ws_bytes,
                   icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(f) row 4, HDBSCAN branch of cluster_pcd (utils_cluster.py:10-29: hdbscan.HDBSCAN(min_cluster_size,
 * min_samples=None, metric='euclidean', alpha=1.0), third-party, environment.yml:57): the part that is
 * O(n^2) on the CPU -- core distances and the minimum spanning tree of the mutual-reachability graph
 *     d(a, b) = max(core(a), core(b), |a - b|),   core(a) = distance to a's min_samples-th nearest
 *     neighbour, a ITSELF COUNTED (tree.query(X, k)[:, -1]: scikit-learn's convention).  The hdbscan package
 *     does not count the point (its boruvka_kdtree path queries k = min_samples + 1, _hdbscan_boruvka.pyx):
 *     pass its min_samples + 1 here -- icp_flow_amd/utils_cluster.py does, for the reference's
 *     HDBSCAN(min_cluster_size, min_samples=None) that is min_cluster_size + 1.
 * The dendrogram, condensed tree and cluster selection on the n - 1 edges are sequential host logic:
 * icpflow_hdbscan_labels below, host C++.  icpflow_cluster_pcd chains the two with the rest of cluster_pcd (row mapping,
 * label histogram, keep rule) inside the library; icp_flow_amd/utils_cluster.py's default path does that rest in numpy.
 *
 * d_points / stride / d_mask as icpflow_dbscan.  cell: edge of the uniform sort grid in metres (speed
 * only; 0.25 suits LiDAR frames).  Outputs: d_edge_a / d_edge_b int32 [n], d_edge_w2 float64 [n]: the
 * n_live - 1 tree edges (caller rows, SQUARED weight, unordered); d_num_edges, d_num_live int32 [1];
 * d_core2 float64 [n] (optional): squared core distance per caller row, NaN for rows that took no part.
 * Exact: ties between equal weights are broken by (smaller row, larger row), so the tree is unique.
 * ------------------------------------------------------------------------- */
size_t icpflow_hdbscan_mst_workspace_bytes(int n);
int icpflow_hdbscan_mst(const float *d_points, int stride, const uint8_t *d_mask, int n, int min_samples, double cell,
                        double *d_core2, int32_t *d_edge_a, int32_t *d_edge_b, double *d_edge_w2,
                        int32_t *d_num_edges, int32_t *d_num_live, void *d_ws, size_t ws_bytes,
                        icpflow_stream_t stream);

/* HOST function (host pointers, no device work, callable without a GPU): HDBSCAN's sequential remainder on
 * the n_points - 1 spanning-tree edges -- what hdbscan.HDBSCAN / sklearn's HDBSCAN do after their spanning tree
 * (sklearn/cluster/_hdbscan/_linkage.pyx make_single_linkage, _tree.pyx tree_to_labels with "eom", no single
 * cluster, epsilon 0): edges (rows of the clustered subset, 0-based; weight = mutual-reachability DISTANCE,
 * i.e. the square root of icpflow_hdbscan_mst's output) -> h_labels int32 [n_points], -1 = noise.
 * Returns ICPFLOW_E_ARG when the edges do not span the points or min_cluster_size < 2. */
int icpflow_hdbscan_labels(const int32_t *h_edge_a, const int32_t *h_edge_b, const double *h_edge_w,
                           int n_points, int min_cluster_size, int32_t *h_labels);

/* ---------------------------------------------------------------------------
 * 8(f) row 10  cluster_pcd as a whole (utils_cluster.py:50-63 with cluster_dbscan :32-48 or hdbscan :10-29): the points of a
 * frame pair in, the labels track() reads out.  The call clusters the STACK of two segments, dst first, as
 * dataset_pca.py:175-182 and demo.py:210-212 stack them -- the caller concatenates nothing; n_src = 0 clusters one cloud.
 *
 * The fields of icpflow_cluster_params_t; icpflow_cluster_default_params fills it with main.py:77-82's defaults and DBSCAN:
 *   method            ICPFLOW_CLUSTER_DBSCAN (utils_cluster.py:32-48) or ICPFLOW_CLUSTER_HDBSCAN (:10-29, --if_hdbscan)
 *   eps               --epsilon: DBSCAN's radius (:35; HDBSCAN does not read it, :14 passes no epsilon)
 *   min_cluster_size  --min_cluster_size: DBSCAN's min_points (:35); HDBSCAN's min_cluster_size (:14), with
 *                     min_samples = min_cluster_size + 1 handed to icpflow_hdbscan_mst (the hdbscan package does not count
 *                     the point itself, see there) -- at most 63
 *   num_clusters      --num_clusters: how many of the largest clusters survive (:19-27, :39-46)
 *   cell              HDBSCAN's sort grid (icpflow_hdbscan_mst), 0 = 0.25
 *
 * d_dst / d_src float32 rows of `stride` floats (x, y, z first); d_mask_dst / d_mask_src uint8 per row or NULL (all rows):
 * rows with mask 0 are the ground rows of cluster_pcd's idxs_nonground (:52-53).
 * Outputs: d_labels_dst [n_dst], d_labels_src [n_src] float32 in cluster_pcd's convention (:54-62): the cluster id, -1 for
 * an unclustered row, -1e8 for a masked row;  d_info int32 [4] = {clusters found, clusters kept, noise rows, live (unmasked)
 * rows}.  "clusters kept" = 0 is where the reference raises IndexError (:24 / :43: nothing left to sort); every label is
 * then -1 or -1e8.
 *
 * The keep rule (:19-27, :39-46), quirks included: the FIRST unique label is dropped unseen -- -1 when at least one row is
 * noise, otherwise cluster 0, which is then never kept; the num_clusters largest of the rest survive.  Named deviation: among
 * clusters of EQUAL size at the cut the LARGER id wins (a stable ascending sort followed by the reference's [::-1]; numpy's
 * default argsort is not stable and its tie order depends on the numpy build).
 *
 * DBSCAN: enqueued work only, like every other entry point -- the keep rule (rank of a cluster = the number of clusters that
 * beat it) and the label finish are kernels.  HDBSCAN: BLOCKING on `stream`: spanning tree and the sort of its edges on the
 * device, one download into host memory the library owns (ICPFLOW_E_HOSTMEM when it cannot be had), icpflow_hdbscan_labels,
 * row mapping / label histogram / keep rule in host C++, one upload, the same finish kernel.  ICPFLOW_E_ARG when fewer than
 * min_cluster_size + 1 rows can be clustered (the hdbscan package raises there).
 * ICPFLOW_E_LIMIT: cluster ids must be exact in float32 -- any n = n_dst + n_src with ceil(n / min_cluster_size) > 2^24.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_CLUSTER_DBSCAN 0
#define ICPFLOW_CLUSTER_HDBSCAN 1
typedef struct icpflow_cluster_params {
    size_t struct_size; /* sizeof(icpflow_cluster_params_t) */
    int method;
    int min_cluster_size;
    int num_clusters;
    int reserved;
    double eps;
    double cell;
} icpflow_cluster_params_t;
int icpflow_cluster_default_params(icpflow_cluster_params_t *params);
size_t icpflow_cluster_pcd_workspace_bytes(int n_dst, int n_src, const icpflow_cluster_params_t *params);
int icpflow_cluster_pcd(const float *d_dst, int n_dst, const float *d_src, int n_src, int stride, const uint8_t *d_mask_dst,
                        const uint8_t *d_mask_src, const icpflow_cluster_params_t *params, float *d_labels_dst,
                        float *d_labels_src, int32_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);

/* icpflow_track_frame from POINTS: icpflow_cluster_pcd of the stack (dst first; main.py:184-215 clusters, then tracks)
 * followed by icpflow_track_frame on the labels it leaves in d_labels_src [n_src] / d_labels_dst [n_dst] (float32, the
 * caller's: the verbose loop, main.py:236-259, reads them).  d_points_* float32 [n,3]; d_mask_* uint8 [n] or NULL.  Every
 * other argument, the results and the scratch protocol (a refusal with *scratch_needed) are icpflow_track_frame's; the
 * scratch holds the clustering's workspace in front of the frame's. */
int icpflow_track_frame_points(const float *d_points_src, const uint8_t *d_mask_src, int n_src, const float *d_points_dst,
                               const uint8_t *d_mask_dst, int n_dst, const icpflow_cluster_params_t *cluster,
                               float *d_labels_src, float *d_labels_dst, const icpflow_registration_t *reg,
                               const icpflow_frame_params_t *par, float *d_rows, float *d_T, int32_t *h_pairs,
                               const float *d_flow_points, const float *d_pose, float *d_flow, void *d_scratch,
                               size_t scratch_bytes, size_t *scratch_needed, icpflow_stream_t stream,
                               const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * 8(f)  ego motion of a LiDAR sequence that comes without poses: scan-to-map odometry resident on the GPU.
 * Replaces: `egomotion` -- utils_ego_motion.py:21-111 with config_kiss_icp.yaml (the reference hands every frame to the
 * third-party kiss_icp package, dataset_pca.py:115-135; this is that METHOD as published, not the package's bits).
 * Poses are float64 [4,4] row-major, column-vector convention (x' = R x + t); poses[j] maps frame j into frame 0's
 * coordinates.  The estimator's second configuration (config_kiss_icp.yaml's "advanced" block: deskew, fixed_threshold) is
 * the icpflow_egomotion_* block below; both are off by default, as in the reference's configuration.
 *
 * Per frame (float32 [n,3] in the sensor's coordinates):
 *   0. deskew        only through icpflow_egomotion_register_frame_stamped with deskew on: every point is moved by
 *                    exp((stamp - mid_stamp) xi), xi = log(inv(pose[-2]) pose[-1]); unchanged with fewer than two poses
 *   1. crop          min_range^2 < x*x + y*y + z*z < max_range^2, evaluated in fp64
 *   2. down-sample   voxel of a coordinate = floor(x / size) in fp64; the point kept in a voxel is the one with the LOWEST
 *                    input index; `frame_ds`: size 0.5 v on the cropped frame, `source`: size 1.5 v on frame_ds
 *                    (v = voxel_size, 0 = max_range / 100); both lists are in ascending input index
 *   3. threshold     sigma = initial_threshold until the sensor has moved more than 5 min_motion_th from frame 0, then
 *                    sqrt(sse / count) over the model deviations of step 6; with a fixed_threshold > 0 sigma is that value
 *                    on every frame (step 6 keeps its books all the same)
 *   4. guess         last_pose * inv(pose[-2]) * pose[-1], identity motion with fewer than two poses
 *   5. registration  of `source` against the map, at most max_iterations Gauss-Newton steps in ONE launch (device-side stop):
 *                    x = T p; correspondence q = the closest map point (fp64 squared distance, first minimum in the order
 *                    voxel offset (dx, dy, dz ascending, dz fastest), then insertion order) among the 27 map voxels around
 *                    floor(x / v), kept if |x - q|^2 < (3 sigma)^2; weight w = (k / (k + |r|^2))^2, k = sigma / 3, r = x - q;
 *                    J = [I | -[x]_x]; (sum w J^T J) dx = -sum w J^T r in fp64, sums in a fixed order; T <- exp(dx) T;
 *                    stop when |dx| < convergence.  Fewer than 3 correspondences, or a dx that is not finite: the loop stops
 *                    without a step (that iteration counts: a source of no points, m = 0, or a map whose voxels were
 *                    all pruned gives the guess, 1 iteration, 0 correspondences -- through register_frame and through
 *                    register_step alike).  Only against a map that has received no frame since the state was created or
 *                    reset is no loop run: the result is the guess, 0 iterations.
 *   6. bookkeeping   deviation D = inv(guess) new_pose adds (|t_D| + 2 max_range sin(theta_D / 2))^2 to sse when that error
 *                    exceeds min_motion_th; frame_ds moved by the new pose (fp64, ((R0 x + R1 y) + R2 z) + t, rounded to
 *                    float32) is added to the map -- voxel size v, at most max_points_per_voxel points per voxel, in input
 *                    order -- and map voxels whose FIRST point is farther than max_range from the new position are dropped.
 *
 * Memory: everything on the device lives in ONE caller-owned buffer of icpflow_ego_state_bytes(params) bytes handed to
 * icpflow_ego_create (the map: two open-addressing tables of map_capacity slots that swap at every prune; the scratch of
 * a frame of at most max_points points).  A frame that does not fit (n > max_points, a table full) is ICPFLOW_E_LIMIT.
 * A state object must not be used by two host threads at once; distinct objects on distinct streams are independent.
 *
 * icpflow_ego_register_frame: steps 1-6, enqueued on `stream` without a host round trip per iteration; BLOCKING at its
 *   end (one read-back per frame: the pose, which the host needs for steps 3, 4 and 6 of the next frame).  h_pose_out
 *   float64 [16].  icpflow_ego_poses: the poses so far.  icpflow_ego_frame_info: float64 [8] of the last frame
 *   (points kept by the crop and frame_ds, points of source, iterations, final |dx|, correspondences of the last
 *   iteration, sigma, live map voxels, 0).
 * The pieces, each asynchronous on `stream`, none touching the odometry (poses, sse); what register_frame chains:
 *   icpflow_ego_downsample   steps 1-2: d_idx_ds / d_idx_source int32 [n] (rows of d_points), d_counts int32 [2]
 *   icpflow_ego_register_step  step 5 alone, stateless: d_source float32 [m,3], h_guess float64 [16], sigma ->
 *                            d_result float64 [20]: pose [16], iterations, final |dx|, correspondences, 0
 *   icpflow_ego_map_add      the map half of step 6 for d_points float32 [n,3] (a frame_ds) under h_pose float64 [16]
 *   icpflow_ego_map_export   the live voxels, unordered: d_keys int64 [capacity] ((ix + 2^20) << 42 | (iy + 2^20) << 21 |
 *                            (iz + 2^20)), d_counts int32 [capacity], d_points float32 [capacity, max_points_per_voxel, 3];
 *                            d_num int32 [1] = number of live voxels (may exceed capacity: the rest was not written)
 * ------------------------------------------------------------------------- */
typedef struct icpflow_ego icpflow_ego_t; /* opaque */
typedef struct icpflow_ego_params {
    size_t struct_size;       /* sizeof(icpflow_ego_params_t) */
    double max_range;         /* 100.0  (config_kiss_icp.yaml data.max_range) */
    double min_range;         /* 1.0    (the reference's setting of data.min_range) */
    double voxel_size;        /* 0 = max_range / 100 (mapping.voxel_size) */
    double min_motion_th;     /* 0.1    (adaptive_threshold.min_motion_th) */
    double initial_threshold; /* 10.0   (adaptive_threshold.initial_threshold; the reference's setting) */
    double convergence;       /* 1e-4   (registration.convergence_criterion) */
    int max_points_per_voxel; /* 20, at most 20 (mapping.max_points_per_voxel) */
    int max_iterations;       /* 500    (registration.max_num_iterations) */
    int max_points;           /* capacity: points of one frame */
    int map_capacity;         /* capacity: slots of each map table, a power of two >= 1024; at most half may be live (a
                               * fuller table, up to every slot, is still CORRECT -- every probe loop ends after
                               * map_capacity steps -- but its chains grow long; one voxel more is ICPFLOW_E_LIMIT) */
} icpflow_ego_params_t;
int icpflow_ego_default_params(icpflow_ego_params_t *params);
size_t icpflow_ego_state_bytes(const icpflow_ego_params_t *params);
int icpflow_ego_create(const icpflow_ego_params_t *params, void *d_mem, size_t mem_bytes, icpflow_stream_t stream,
                       icpflow_ego_t **out);
int icpflow_ego_destroy(icpflow_ego_t *ego);
int icpflow_ego_reset(icpflow_ego_t *ego, icpflow_stream_t stream);
int icpflow_ego_register_frame(icpflow_ego_t *ego, const float *d_points, int n, double *h_pose_out, icpflow_stream_t stream);
int icpflow_ego_poses(const icpflow_ego_t *ego, double *h_poses, int capacity, int *h_count);
int icpflow_ego_frame_info(const icpflow_ego_t *ego, double *h_info);
int icpflow_ego_downsample(icpflow_ego_t *ego, const float *d_points, int n, int32_t *d_idx_ds, int32_t *d_idx_source,
                           int32_t *d_counts, icpflow_stream_t stream);
int icpflow_ego_register_step(icpflow_ego_t *ego, const float *d_source, int m, const double *h_guess, double sigma,
                              double *d_result, icpflow_stream_t stream);
int icpflow_ego_map_add(icpflow_ego_t *ego, const float *d_points, int n, const double *h_pose, icpflow_stream_t stream);
int icpflow_ego_map_export(icpflow_ego_t *ego, int64_t *d_keys, int32_t *d_counts, float *d_points, int capacity,
                           int32_t *d_num, icpflow_stream_t stream);

/* 8(f), second configuration: motion compensation ("deskewing") by per-point stamps, and a fixed threshold.
 * Replaces: the motion compensator the reference's estimator calls on every frame with `deskew: True`
 * (utils_ego_motion.py:29, :54) and `fixed_threshold` of the same block; restated from the published method.
 *
 * Step 0.  xi = (rho, omega) = log(inv(pose[-2]) pose[-1]) on the host in fp64.  Point i with stamp s_i: d = s_i - mid_stamp,
 * p_i' = R p_i + V (d rho), R | V (d rho) = exp(d xi): with theta = |d omega|, K = [d omega]_x
 *     R = I + (sin theta / theta) K + ((1 - cos theta) / theta^2) K^2
 *     V = I + ((1 - cos theta) / theta^2) K + ((theta - sin theta) / theta^3) K^2
 * evaluated per point in fp64 in a fixed order from the unit axis' K and K^2 scaled by the signed angle phi = d |omega|
 * (one sincos, of phi / 2: sin phi = 2 s c and 1 - cos phi = 2 s s carry no cancellation), rounded ONCE to float32.  The
 * two coefficients that divide by phi, (1 - cos phi) / phi and (phi - sin phi) / phi, come from their series
 * phi (1/2 - phi^2 / 24) and phi^2 (1/6 - phi^2 / 120) for |phi| < 2^-13: there the series' next term is below 2^-54 of
 * the coefficient, and the closed forms differ from the series by less than 2^-52 of the order-1 entries of V they add to,
 * i.e. both branches give the coordinates to fp64 rounding.  The log reads the axis off the skew part of the rotation
 * (angle = atan2(|skew|, (trace - 1) / 2)): two poses a half turn apart have no twist and are ICPFLOW_E_ARG.
 * Stamps are used AS GIVEN: the caller normalises them to [0, 1] over the sweep (mid_stamp 0.5 = the middle of the sweep is
 * where the frame's pose holds).  A stamp that is not finite gives a row that is not finite, which the crop of step 1
 * drops (its comparisons are false).
 *
 * icpflow_egomotion_default_params: deskew 0, mid_stamp 0.5, fixed_threshold 0 (= adaptive).
 * icpflow_egomotion_set_params: host only, no launch; the settings are kept across icpflow_ego_reset.  mid_stamp and
 *   fixed_threshold must be finite and >= 0, deskew 0 or 1.
 * icpflow_egomotion_deskew: step 0 alone, a piece like those above: asynchronous on `stream`, poses and sse untouched.
 *   d_points float32 [n,3], d_stamps float32 [n] -> d_out float32 [n,3] (must not overlap d_points).  h_poses float64
 *   [2][16] = (pose[-2], pose[-1]) to interpolate between, read before the call returns; NULL = the state's last two poses,
 *   and with fewer than two of those d_out is a copy of d_points.
 * icpflow_egomotion_register_frame_stamped: step 0 into d_corrected (float32 [n,3], the caller's: the state keeps its
 *   size), then steps 1-6 on d_corrected exactly as icpflow_ego_register_frame runs them; on return d_corrected holds the
 *   corrected frame.  With deskew 0 or d_stamps NULL it IS icpflow_ego_register_frame on d_points, bit for bit, and
 *   d_corrected may be NULL; with deskew on, stamps given and d_corrected NULL it is ICPFLOW_E_ARG before anything is
 *   enqueued. */
typedef struct icpflow_ego_motion_params {
    size_t struct_size;     /* sizeof(icpflow_ego_motion_params_t) */
    int deskew;             /* 0      (config_kiss_icp.yaml data.deskew) */
    int reserved;           /* 0 */
    double mid_stamp;       /* 0.5    the stamp at which the frame's pose holds */
    double fixed_threshold; /* 0 = adaptive (adaptive_threshold.fixed_threshold) */
} icpflow_ego_motion_params_t;
int icpflow_egomotion_default_params(icpflow_ego_motion_params_t *params);
int icpflow_egomotion_set_params(icpflow_ego_t *ego, const icpflow_ego_motion_params_t *params);
int icpflow_egomotion_deskew(icpflow_ego_t *ego, const float *d_points, const float *d_stamps, int n, const double *h_poses,
                             float *d_out, icpflow_stream_t stream);
int icpflow_egomotion_register_frame_stamped(icpflow_ego_t *ego, const float *d_points, const float *d_stamps, int n,
                                             float *d_corrected, double *h_pose_out, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(f)  evaluation of a whole sequence (a Waymo / nuScenes sample of the reference: m points of F frames, frame j = the
 * rows with time_indice == j) by the reference's metric protocol, without the points or the flows crossing to the host.
 * All arrays are row-major and contiguous; points and the ground truth are float64 (a float32 sample is widened by the
 * caller: exact), labels and time indices int32, poses float64 [4,4] row-major in the column-vector convention.
 *
 * icpflow_seq_gt_flow -- replaces utils_loading.py:21-31 (ego_motion_compensation), :33-48 (reconstruct_sequence) and the
 *   subtraction of dataset_pca.py:66-69.  Per row, in fp64, every operation rounded by itself
 *   (((R0 x + R1 y) + R2 z) + t per coordinate):
 *       p_ego  = R_ego[t] p + t_ego[t]                     d_ego [F,4,4]; NULL = this step is skipped
 *       p_full = R_inst[inst * F + t] p_ego + t_inst[..]   d_inst_tsfm [K,F,4,4], inst = d_inst_labels[row]; NULL = skipped
 *       out    = p_full - p (ICPFLOW_SEQ_OUT_FLOW: the scene flow) or p_full (ICPFLOW_SEQ_OUT_POINTS: what the two functions
 *                of the reference return, one step each)
 *   d_out float64 [m,3].  A row with t outside [0, F) or inst outside [0, K) is NOT computed: nothing is written for it and
 *   it is counted in d_bad_rows (int64 [1]).  numpy's wrap-around of a negative index (tsfm[-1] is the last pose) is NOT
 *   reproduced, and inst and t are checked each by itself, where the reference checks only their combination inst * F + t.
 *
 * icpflow_seq_metrics -- replaces utils_eval.py:24-63 (crop_data), :162-180 (compute_epe_test's per-point part) and the
 *   masks and sums of :185-368 (calculate_metrics); the meters' arithmetic on the resulting table is host code
 *   (icp_flow_amd/utils_eval.py).  One pass over the rows.  A row is kept (utils_eval.py:33-38) when
 *       crop = ICPFLOW_SEQ_CROP_NONE: always          (calculate_metrics with eval_ground, which does not crop at all)
 *       crop = ICPFLOW_SEQ_CROP_XY:   |x| < range_x and |y| < range_y                      (crop_data with eval_ground)
 *       crop = ICPFLOW_SEQ_CROP_XYZ:  ... and z > z_min, z_min = range_z + ground_slack    (crop_data without)
 *   -- thresholds as the caller rounds them: numpy compares a float32 coordinate with the float32-rounded threshold.
 *   Per kept row, in fp64 with numpy's operation order: d = gt - pred (d_pred_flow float32 [m,3], as the flow kernel leaves
 *   it; widened), e = sqrt((dx dx + dy dy) + dz dz), r = e / (sqrt((gx gx + gy gy) + gz gz) + 1e-20), the square root
 *   correctly rounded and the division IEEE; nothing is contracted into a fused multiply-add.  Predicates
 *   (utils_eval.py:170-180): e < 0.05 or r < 0.05;  e < 0.1 or r < 0.1;  e > 0.3 or r > 0.1;  e > 0.3 and r > 0.3.
 *   d_table int64 [F][6][6]: row j = 1 .. F-1 is gap j (the kept rows with time index j), row 0 the sum of the gap rows (the
 *   reference's rows 0 and F: every kept point of a frame other than 0); classes in the order overall, static (sd == 0),
 *   static_bg (sd == 0 and fb == 0), static_fg (sd == 0 and fb == 1), dynamic (sd == 1), dynamic_fg (sd == 1 and fb == 1) --
 *   a row whose labels are neither 0 nor 1 counts in `overall` only; values: number of rows, sum of e (the BITS OF A
 *   float64 in the int64 word), and the number of rows satisfying each of the four predicates.
 *   d_info int64 [2]: the kept rows of frame 0 (utils_eval.py:275 weights `overall_0` with len(flow_seq), which includes
 *   them), and the rows whose time index is outside [0, F) (counted nowhere else).
 *   Counts are exact.  The sums of e are a function of the arguments alone -- not of the device, the stream or the
 *   scheduling: a fixed reduction order, no floating-point atomics (csrc/seqeval.hip).  F > ICPFLOW_SEQ_MAX_FRAMES is
 *   ICPFLOW_E_LIMIT (the table of a workgroup lives in LDS).
 *
 * icpflow_seq_argo_sample -- replaces dataset_argo.py:47-50 (the gathers), :66-71 (the two labels) and :83-89 (the
 *   two-frame sample) for one Argoverse 2 file as ZeroFlow exports it, without the clouds or the flow crossing to the
 *   host.  d_pc1 [n1,3], d_pc2 [n2,3] in points_dtype, d_flow_0_1 [n1,3] in flow_dtype (ICPFLOW_DTYPE_FLOAT32 or _FLOAT64:
 *   the file's own types), d_classes1 float64 [n1] (widened by the caller: exact for every integer or float type an npz
 *   holds, and == then decides as numpy does on the file's type), d_valid1 int64 [m1], d_valid2 int64 [m2]: the files'
 *   pc*_flows_valid_idx (a boolean mask is the caller's np.flatnonzero).  Outputs of m = m2 + m1 rows:
 *       rows [0, m2)   frame 0: d_points = pc2[valid2[i]] widened, d_time_indice 0, d_sd_labels 0, d_fb_labels 0, zero flow
 *       rows [m2, m)   frame 1: d_points = pc1[valid1[k]] widened, d_time_indice 1, d_scene_flow = flow[valid1[k]] widened,
 *                      sd = (|flow row| > sd_threshold), fb = 1 except where the class equals -1 or one of the
 *                      n_background entries of h_background (HOST memory, read before the call returns), there 0
 *   |flow row| is np.linalg.norm(flow, axis=-1) as numpy computes it IN flow_dtype: sqrt((x x + y y) + z z), every
 *   operation rounded by itself, the square root correctly rounded; the caller passes sd_threshold as numpy compares it,
 *   0.5 * 0.1 rounded to flow_dtype.  A NaN norm is not > threshold (sd = 0), a NaN class equals nothing (fb = 1).
 *   An index outside [0, n) writes nothing for its row and is counted in d_bad_rows (int64 [1]); numpy's wrap-around of a
 *   negative index is NOT reproduced.  Rows of the inputs that no index selects are never read (the files pad them with
 *   non-finite values).  No workspace.  n_background > ICPFLOW_ARGO_MAX_BACKGROUND is ICPFLOW_E_LIMIT; a null pointer, a
 *   negative size or an unknown dtype is ICPFLOW_E_ARG before any launch; m = 0 succeeds (*d_bad_rows = 0).  Asynchronous
 *   on `stream`; the results are a function of the arguments alone.
 *
 * icpflow_seq_class_table -- what everyone who reports on Argoverse 2 reports, and what the reference carries the tables for
 *   without using them (dataset_argo.py:145-217: category names, meta categories, speed buckets, end-point-error splits):
 *   counts and sums per class, speed bucket and error split, in one more pass over the rows of a sample.  d_points,
 *   d_time_indice, d_gt_flow, d_pred_flow, m, F, crop, range_x, range_y, z_min: as for icpflow_seq_metrics, with the same row
 *   test (one __device__ function, csrc/rowerr.hpp).  A row counts when it passes the crop and its time index is in [1, F);
 *   there is no axis for gaps.  d_info int64 [2]: the kept rows of frame 0, and the rows with a time index outside [0, F).
 *   Per counted row:
 *       class row     g = v - class_lo when v = d_classes[row] (float64 [m]) is integer-valued and class_lo <= v <= class_lo + G - 2;
 *                     everything else -- NaN, +-inf, 3.5, a value out of range -- is row G - 1, "other"
 *       speed bucket  s = the number of h_speed_edges[k], k < S - 1, with |gt| >= edge: S buckets [lo, hi) from S - 1 interior
 *                     edges in metres per frame; |gt| = sqrt((x x + y y) + z z) in fp64, every operation rounded by itself
 *       error split   the same count of h_error_edges[k], k < E - 1, with e >= edge; e is icpflow_seq_metrics' per-row e
 *   (a NaN is >= nothing: bucket / split 0).  The edge arrays live in HOST memory and are read before the call returns; they
 *   must be finite and strictly ascending; NULL is accepted for a list of no edges (S = 1, E = 1).  class_lo is an integer value.
 *   d_table int64 [G][S][E + 2]: words 0 .. E-1 the rows per error split, word E the BITS OF the float64 sum of e, word E + 1
 *   the bits of the float64 sum of |gt|.
 *   G <= ICPFLOW_CLASS_MAX_ROWS, S and E <= ICPFLOW_CLASS_MAX_BUCKETS and G * S * (E + 2) <= ICPFLOW_CLASS_MAX_WORDS, else
 *   ICPFLOW_E_LIMIT (a wave keeps its own cells in LDS: four waves x 1024 words x 8 bytes = 32 KB; the Argoverse 2 call needs
 *   33 x 3 x 5 = 495 words).  A null pointer, a negative size, F < 1, G < 2, S < 1, E < 1, unsorted or non-finite edges are
 *   ICPFLOW_E_ARG before any launch.  The workspace is the caller's: icpflow_seq_class_table_workspace_bytes(m, G, S, E) bytes
 *   (0 for arguments the call refuses), 8-byte aligned; nothing in it is read before it is written; fewer bytes are
 *   ICPFLOW_E_WORKSPACE before anything is written.  m = 0 succeeds with a zero table.  Counts are exact; the two sums of a
 *   cell are a function of the arguments alone -- fixed reduction order, no floating-point atomics (csrc/classeval.hip).
 *   Asynchronous on `stream`.
 *
 * icpflow_seq_bucket_table -- the cells behind the bucket-normalised EPE Argoverse 2 has been ranked by since its 2024
 *   challenge (Khatri et al., "I Can't Believe It's Not Scene Flow!", ECCV 2024), which the reference has no code for: per
 *   class row and speed bucket the rows, the sum of e and the sum of |gt|, in one more pass over the rows of a sample.  Every
 *   argument it shares with icpflow_seq_class_table means what it means there, word for word: the row test, the rows that
 *   count (crop passed, time index in [1, F)), d_info, the class row of a value (not integer-valued or outside
 *   [class_lo, class_lo + G - 2]: row G - 1) and the speed bucket (the number of h_speed_edges[k], k < S - 1, with
 *   |gt| >= edge; a NaN is bucket 0) are the same __device__ functions (csrc/rowerr.hpp).  There is no error split.
 *   d_table int64 [G][S][3]: word 0 the rows of the cell, word 1 the BITS OF the float64 sum of e, word 2 the bits of the
 *   float64 sum of |gt|.  The metric itself -- per class the static EPE of bucket 0 and the mean over the non-empty buckets
 *   b >= 1 of (sum of e) / (sum of |gt|) -- is host arithmetic on the table, as are the protocol's 50 edges and its grouping
 *   of the rows into classes (icp_flow_amd/utils_eval.py: bucketed_epe, ARGO_BUCKET_EDGES, ARGO_CHALLENGE_GROUPS).
 *   G <= ICPFLOW_BUCKET_MAX_ROWS and S <= ICPFLOW_BUCKET_MAX_BUCKETS, else ICPFLOW_E_LIMIT: a WORKGROUP keeps one table in
 *   dynamic LDS, 64 x 64 x 3 words = 96 KB at the limits (the Argoverse 2 call needs 33 x 51 x 3 = 5049 words, beyond what
 *   icpflow_seq_class_table's table per wave holds).  A null pointer, a negative size, F < 1, G < 2, S < 1, a class_lo that is
 *   no integer value, unsorted or non-finite edges are ICPFLOW_E_ARG before any launch.  The workspace is the caller's:
 *   icpflow_seq_bucket_table_workspace_bytes(m, G, S) = grid(m) * (G * S * 3 + 2) * 8 bytes rounded up to a multiple of 256,
 *   grid(m) = ceil(m / 2048) clamped to [1, 256] (0 for arguments the call refuses), 8-byte aligned; nothing in it is read
 *   before it is written; fewer bytes are ICPFLOW_E_WORKSPACE before anything is written.  m = 0 succeeds with a zero table.
 *   Counts are exact; the two sums of a cell are a function of the arguments alone -- fixed reduction order, no
 *   floating-point atomics (csrc/bucketeval.hip).  Asynchronous on `stream`, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_SEQ_MAX_FRAMES 16
#define ICPFLOW_SEQ_OUT_FLOW 0
#define ICPFLOW_SEQ_OUT_POINTS 1
#define ICPFLOW_SEQ_CROP_NONE 0
#define ICPFLOW_SEQ_CROP_XY 1
#define ICPFLOW_SEQ_CROP_XYZ 2
size_t icpflow_seq_gt_flow_workspace_bytes(int m);
int icpflow_seq_gt_flow(const double *d_points, const int32_t *d_time_indice, const int32_t *d_inst_labels, int m,
                        const double *d_ego, int F, const double *d_inst_tsfm, int K, int output, double *d_out,
                        int64_t *d_bad_rows, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);
size_t icpflow_seq_metrics_workspace_bytes(int m, int F);
int icpflow_seq_metrics(const double *d_points, const int32_t *d_time_indice, const int32_t *d_sd_labels,
                        const int32_t *d_fb_labels, const double *d_gt_flow, const float *d_pred_flow, int m, int F, int crop,
                        double range_x, double range_y, double z_min, int64_t *d_table, int64_t *d_info, void *d_ws,
                        size_t ws_bytes, icpflow_stream_t stream);
#define ICPFLOW_DTYPE_FLOAT32 0
#define ICPFLOW_DTYPE_FLOAT64 1
#define ICPFLOW_ARGO_MAX_BACKGROUND 64
int icpflow_seq_argo_sample(const void *d_pc1, int n1, const void *d_pc2, int n2, int points_dtype, const void *d_flow_0_1,
                            int flow_dtype, const double *d_classes1, const int64_t *d_valid1, int m1, const int64_t *d_valid2,
                            int m2, const int32_t *h_background, int n_background, double sd_threshold, double *d_points,
                            int32_t *d_time_indice, int32_t *d_sd_labels, int32_t *d_fb_labels, double *d_scene_flow,
                            int64_t *d_bad_rows, icpflow_stream_t stream);
#define ICPFLOW_CLASS_MAX_ROWS 64
#define ICPFLOW_CLASS_MAX_BUCKETS 8
#define ICPFLOW_CLASS_MAX_WORDS 1024
size_t icpflow_seq_class_table_workspace_bytes(int m, int G, int S, int E);
int icpflow_seq_class_table(const double *d_points, const int32_t *d_time_indice, const double *d_classes,
                            const double *d_gt_flow, const float *d_pred_flow, int m, int F, int crop, double range_x,
                            double range_y, double z_min, double class_lo, int G, const double *h_speed_edges, int S,
                            const double *h_error_edges, int E, int64_t *d_table, int64_t *d_info, void *d_ws,
                            size_t ws_bytes, icpflow_stream_t stream);
#define ICPFLOW_BUCKET_MAX_ROWS 64
#define ICPFLOW_BUCKET_MAX_BUCKETS 64
size_t icpflow_seq_bucket_table_workspace_bytes(int m, int G, int S);
int icpflow_seq_bucket_table(const double *d_points, const int32_t *d_time_indice, const double *d_classes,
                             const double *d_gt_flow, const float *d_pred_flow, int m, int F, int crop, double range_x,
                             double range_y, double z_min, double class_lo, int G, const double *h_speed_edges, int S,
                             int64_t *d_table, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(f)  per-segment evaluation of one labelled cloud of one frame pair: the numbers behind the reference's verbose loop,
 * without the flows crossing to the host.
 *
 * icpflow_seq_segment_table -- replaces the per-segment masks and reductions of utils_flow.py:86-95 (idx_i, idx_j,
 *   compute_epe_test of the segment's rows), :110 (len_i, len_j, mean_i, mean_j), :123 (mean(x + flow), mean(x)), on the
 *   rows utils_debug.py:37-46 keeps.  A segment is one distinct value of d_labels (float32 [n]); segments appear in ascending
 *   order exactly as icpflow_cluster_table defines them (its dictionary and stable order are reused): ground (-1e8) and
 *   noise (-1) are segments like any other, Lmax <= 4096 (else ICPFLOW_E_LIMIT), and *d_num (int32) is the number of
 *   segments, or the NEGATIVE count when there are more distinct labels than Lmax (nothing of the table is written then).
 *   A row is kept when z > z_min (-inf: no crop; the caller rounds the threshold to the points' stored dtype, as for
 *   icpflow_seq_metrics).  d_points float64 [n,3], d_gt_flow float64 [n,3], d_pred_flow float32 [n,3].  Per kept row e, r and
 *   the four predicates are icpflow_seq_metrics' per-row arithmetic (one __device__ function, csrc/rowerr.hpp).
 *   d_table double [Lmax][ICPFLOW_SEG_COLS], row c = the c-th distinct label (rows from *d_num on are not written):
 *       0       label                                1       rows of the segment
 *       2       kept rows                            3       sum of e over the kept rows
 *       4 - 7   kept rows satisfying each predicate (strict, relax, outlier, Routlier)
 *       8 - 10  sum x, sum y, sum z over the kept rows
 *       11 - 13 sum (x + fx), (y + fy), (z + fz), f the predicted flow widened to fp64, each term rounded once
 *       14 - 15 zero
 *   Counts are exact in a double.  With d_gt_flow == NULL and d_pred_flow == NULL only columns 0 - 2 and 8 - 10 are filled
 *   (the others are zero): the destination cloud, for len_j and mean_j.  Exactly one of the two NULL is ICPFLOW_E_ARG.
 *   Every sum is a function of the arguments alone: segments are cut into chunks of 1024 rows of the stable order, a
 *   workgroup per chunk (a large segment does not serialise on one wave), fixed order inside the chunk, chunks added in
 *   ascending order; no floating-point atomics (csrc/segeval.hip).
 *   The workspace is the caller's: icpflow_seq_segment_table_workspace_bytes(n, Lmax) bytes (0 for arguments the call
 *   refuses), 8-byte aligned; nothing in it is read before it is written; fewer bytes are ICPFLOW_E_WORKSPACE before anything
 *   is written.  n == 0 succeeds with *d_num = 0.  Asynchronous on `stream`.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_SEG_COLS 16
size_t icpflow_seq_segment_table_workspace_bytes(int n, int Lmax);
int icpflow_seq_segment_table(const double *d_points, const float *d_labels, int n, const double *d_gt_flow,
                              const float *d_pred_flow, double z_min, double *d_table, int Lmax, int32_t *d_num, void *d_ws,
                              size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(g)  nearest-neighbour residual: flow judged without ground truth.  No counterpart in the reference: the truncated
 * nearest-neighbour (Chamfer) distance of label-free scene-flow work (COVERAGE.md, named deviations).
 *
 * icpflow_nn_residual -- one direction.  Queries d_query float32 [n,3], optional d_flow float32 [n,3] (NULL: no warp),
 *   targets d_target float32 [m,3], radius r in metres, in [1e-3, 1e3] (else ICPFLOW_E_ARG).
 *   Arithmetic, every operation rounded by itself (the library is built with -ffp-contract=off): q = p + f, one fp32 addition
 *   per coordinate; r2 = (float)r * (float)r, rounded once on the host; d2(q, t) = (dx dx + dy dy) + dz dz in fp32 with
 *   dx = q.x - t.x; a target is a HIT iff d2 <= r2.  Per query d_d2_out float32 [n] is the minimum d2 over the hits and
 *   d_idx_out int32 [n] its target row, the LOWEST row on equal d2; with no hit idx = -1 and d2 = r2.
 *   Bad rows: a target with a non-finite coordinate or one beyond +-1e6 m (the pad rows (1e8, 1e8, 1e8) among them) is never a
 *   neighbour; a query whose q has such a coordinate, or whose group lies outside [0, G), gets idx = -2, d2 = r2 and enters
 *   no cell of the table.
 *   The search is exact: a hashed uniform grid of cell edge 1.01 r over the targets (cell = floor((double)v / h) in fp64,
 *   H = 2^k >= 2 m buckets), built by count / exclusive scan / scatter over several workgroups, and the 27 cells around q
 *   (csrc/nnresid.hip states why no hit lies outside them); the queries are binned by the same cells, so that a wave's lanes
 *   walk the same buckets.  Every output is a function of the arguments alone, whatever order the scatter leaves inside a
 *   bucket.
 *   d_group int32 [n] (NULL: every row in group 0), 1 <= G <= ICPFLOW_NNR_MAX_GROUPS; h_edges (HOST) E <= ICPFLOW_NNR_MAX_EDGES
 *   distances in metres: finite, positive, strictly ascending, at most r.  d_table int64 [G][E + 4], per group: word 0 the good
 *   rows, word 1 the hits, words 2 .. E + 1 the rows with d <= edge, word E + 2 the BITS OF the float64 sum of d, word E + 3
 *   the bits of the float64 sum of d * d; d = sqrtf(d2_out) in fp32, correctly rounded, then widened (a miss counts with
 *   d = sqrtf(r2): the distance is truncated at the radius), the edge test compares the widened d with the fp64 edge, d * d is
 *   the exact fp64 product.  Counts are exact; the sums have a fixed order and no floating-point atomics.
 *   d_info int64 [4], required: bad queries, bad targets, occupied buckets, the longest bucket (the last two are diagnostics).
 *   d_d2_out, d_idx_out and d_table may each be NULL, not all three.  A null pointer, a negative size, r, G or E outside
 *   their ranges, bad edges are ICPFLOW_E_ARG, n or m > 2^29 is ICPFLOW_E_LIMIT, before any launch.  The workspace is the
 *   caller's, 16-byte aligned: icpflow_nn_residual_workspace_bytes(n, m, G, E) =
 *       table(m) + table(n) + 2 a(4 n) + a(8 grid(n) G (E + 4)),   table(k) = 2 a(4 H) + 4 a(4 ceil(H / 1024)) + 256 + a(16 k)
 *   bytes, a(x) = x rounded up to a multiple of 256, H the smallest power of two >= max(2 k, 1), grid(n) = ceil(n / 2048)
 *   clamped to [1, 256] (0 for sizes the call refuses).  Nothing in it is read before it is written; fewer bytes are
 *   ICPFLOW_E_WORKSPACE before anything is written.  n = 0 and m = 0 succeed (m = 0: every good query is a miss).
 *   Asynchronous on `stream`, no host synchronisation, no allocation.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_NNR_MAX_GROUPS 64
#define ICPFLOW_NNR_MAX_EDGES 4
size_t icpflow_nn_residual_workspace_bytes(int n, int m, int G, int E);
int icpflow_nn_residual(const float *d_query, const float *d_flow, int n, const float *d_target, int m, double radius,
                        const int32_t *d_group, int G, const double *h_edges, int E, float *d_d2_out, int32_t *d_idx_out,
                        int64_t *d_table, int64_t *d_info, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(g)  the residual per segment, before and after the flow: which cluster was registered wrongly, without ground truth.
 *
 * icpflow_nn_residual_segments -- two queries against ONE grid.  d_before float32 [n,3] (the ego-compensated source), d_after
 *   float32 [n,3] (the cloud the flow applies to; may be the same pointer as d_before), d_flow float32 [n,3] or NULL: the AFTER
 *   query is q = d_after + d_flow, one fp32 addition per coordinate (NULL: q = d_after); the BEFORE query is d_before as it
 *   is.  d_target float32 [m,3], d_labels float32 [n], radius in [1e-3, 1e3], h_edges (HOST) E <= ICPFLOW_NNR_MAX_EDGES edges:
 *   finite, positive, strictly ascending, at most the radius.
 *   The arithmetic, the hit rule (d2 <= r2), the bad-row rule and the exact search are icpflow_nn_residual's, word for word:
 *   the same device functions (csrc/nnresid.hpp), no copy.  The grid over the target is built once; each side's queries are
 *   binned and run through the binned query kernel.  d_d2_before and d_d2_after float32 [n] may each be NULL; where given they
 *   equal, bit for bit, what two icpflow_nn_residual calls write to d_d2_out.
 *   A segment is one distinct value of d_labels, in ascending order, exactly as icpflow_cluster_table defines it (its dictionary
 *   and stable order are reused: -0.0 and +0.0 are one label, NaN labels one segment per bit pattern); Lmax <= 4096 (else
 *   ICPFLOW_E_LIMIT); *d_num (int32) is the number of segments, or the NEGATIVE count when there are more distinct labels than
 *   Lmax (nothing of the table is written then).
 *   d_table double [Lmax][ICPFLOW_NNRS_COLS], row c = the c-th label (rows from *d_num on are not written):
 *       0        label                                1        rows of the segment
 *       2 - 9    BEFORE: good rows, hits, rows with d <= edge[k] (k < 4; zero for k >= E), sum of d, sum of d * d
 *       10 - 17  AFTER: the same eight
 *   d = sqrtf(d2) widened to fp64, the edge test and d * d as in icpflow_nn_residual's table; a miss counts with sqrtf(r2); a
 *   bad query enters nothing on its side.  Counts are exact in a double.
 *   Every number is a function of the arguments alone, by icpflow_seq_segment_table's scheme: segments cut into chunks of 1024
 *   rows of the stable order, a workgroup of 256 threads per chunk, thread t takes rows t, t + 256, t + 512, t + 768 in that
 *   order, counts by ballot and popcount, sums through one fixed butterfly with the waves added in wave order, the chunks added
 *   in ascending order; no floating-point atomics (csrc/segresid.hip).
 *   d_info int64 [6], required: bad queries before, bad queries after, bad targets, occupied buckets, the longest bucket, 0.
 *   Refusals, all before any launch: a null required pointer, a negative size, Lmax < 1, a radius, E or edges outside their
 *   ranges are ICPFLOW_E_ARG; n or m > 2^29 or Lmax > 4096 are ICPFLOW_E_LIMIT; fewer workspace bytes than the query says are
 *   ICPFLOW_E_WORKSPACE before anything is written; a workspace that is not 16-byte aligned is ICPFLOW_E_ARG.  n = 0 succeeds
 *   with *d_num = 0; m = 0 succeeds (every good query is a miss).
 *   The workspace is the caller's: icpflow_nn_residual_segments_workspace_bytes(n, m, Lmax, E) =
 *       table(m) + table(n) + 3 a(4 n) + a(8 n) + a(72 Lmax) + a(4 (Lmax + 1)) + a(128 chunks) + a(T)
 *   bytes: table(k) and a(x) as for icpflow_nn_residual (ONE query grid, table(n): the AFTER side is binned into it once the
 *   BEFORE side's query is through), two d2 arrays and one idx array, the stable order, the segments' (label, count, start)
 *   rows, the first chunk of every segment, chunks = floor(n / 1024) + min(n, Lmax) + 1 partials of 2 x 8 doubles, and
 *   T = icpflow_cluster_table_workspace_bytes(max(n, 1), Lmax), the label order's own workspace.  E does not enter; 0 for
 *   arguments the call refuses.  Nothing in it is read before it is written.  Asynchronous on `stream`, no host
 *   synchronisation, no allocation.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_NNRS_COLS 18
size_t icpflow_nn_residual_segments_workspace_bytes(int n, int m, int Lmax, int E);
int icpflow_nn_residual_segments(const float *d_before, const float *d_after, const float *d_flow, const float *d_labels, int n,
                                 const float *d_target, int m, double radius, const double *h_edges, int E, double *d_table,
                                 int Lmax, int32_t *d_num, float *d_d2_before, float *d_d2_after, int64_t *d_info, void *d_ws,
                                 size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(h)  line of sight: a missing neighbour told apart -- contradicted by the destination sweep, or merely unobserved.  No
 * counterpart in the reference: the free-space / visibility test of label-free scene-flow work (COVERAGE.md, named deviations).
 * A LiDAR return certifies the ray in front of it as empty: a warped source point in FRONT of the nearest return along its ray
 * sits in space the destination sweep saw through (evidence against the flow); one behind it, on a ray without a return or
 * outside the field of view is unobserved (it excuses a missing neighbour).
 *
 * The pixel map.  No transcendental function; every operation below is ONE fp32 operation rounded by itself (the library is
 * built with -ffp-contract=off, IEEE division and correctly rounded sqrtf).  The parameters and the origin o (HOST double[3],
 * finite, within 1e6 m) are narrowed to float once, on the host; rs = (float)H / (tan_hi - tan_lo) in fp32, once.  For a point v:
 *     u = v - o per coordinate;  h2 = ux ux + uy uy;  d2 = h2 + uz uz;  rho = sqrtf(d2)
 *     column, by the diamond angle (monotone around the circle, one division):  s = |ux| + |uy|,  g = uy / s,
 *         p = g where ux >= 0 and uy >= 0;  p = 4 + g where ux >= 0 and uy < 0;  p = 2 - g where ux < 0  (-0.0 counts as >= 0)
 *         col = (int)floorf(p * (float)(W / 4));  col == W (p rounded to 4) wraps to 0
 *     row, by the tangent of the elevation:  t = uz / sqrtf(h2),  row = (int)floorf((t - tan_lo) * rs);  row == H (rounding)
 *         becomes H - 1
 *     OUTSIDE (no pixel): s == 0, or !(t >= tan_lo && t < tan_hi) (an infinite or NaN t too), or rho < min_range, or
 *         rho > max_range
 *   A BAD row is icpflow_nn_residual's, word for word (the same device function): a non-finite coordinate or one beyond
 *   +-1e6 m; it is never a target and never classified.
 *
 * icpflow_sight_params_t: W a multiple of 4 in [4, 8192], H in [1, 2048], W * H <= 2^22; tan_lo < tan_hi, finite (compared as
 *   floats); 0 <= min_range < max_range <= 1e6 (as floats); margin_abs >= 0, 0 <= margin_rel < 1.  Anything else, or a
 *   struct_size that is not sizeof(icpflow_sight_params_t), is ICPFLOW_E_ARG.  icpflow_sight_default_params fills the defaults
 *   (COVERAGE.md row 15 says where they come from).
 *
 * icpflow_sight_build -- the depth image of one destination sweep, d_target float32 [m,3].  d_image is the caller's, uint32
 *   [2][H][W], all of it written.  Plane 0: per pixel the BITS of the smallest rho of the targets in it, the bits of +inf
 *   (0x7f800000) in an empty pixel -- non-negative floats order like their bits, so this is an integer atomicMin, which does not
 *   depend on the order of arrival; no floating-point atomic.  Plane 1: per pixel the minimum of plane 0 over the 3 x 3 pixels
 *   around it, columns modulo W, rows clipped to [0, H) -- a point correctly placed on an object's silhouette falls into a
 *   pixel that may hold background only.  d_info int64 [3], required: bad targets, targets OUTSIDE, occupied pixels of plane 0.
 *   Three launches (fill, scatter, 3 x 3), no workspace.  m = 0 succeeds and leaves an empty image; m < 0 and null pointers are
 *   ICPFLOW_E_ARG, m > 2^29 is ICPFLOW_E_LIMIT, before any launch.
 *
 * icpflow_sight_query -- the ray test of n rows against an image built with the SAME params and origin.  q = d_query + d_flow,
 *   one fp32 addition per coordinate (d_flow NULL: q = d_query); rho and the pixel of q by the map above; n9 = plane 1 at the
 *   pixel; thr = margin_abs + margin_rel * rho (two fp32 operations).  d_code_out int32 [n]:
 *       -2  a bad row                             ICPFLOW_SIGHT_OUTSIDE 0          no pixel
 *       ICPFLOW_SIGHT_NO_RETURN 1      n9 == +inf           ICPFLOW_SIGHT_SEEN_THROUGH 2     rho + thr < n9
 *       ICPFLOW_SIGHT_AT_FIRST_RETURN 3  not 2, and rho - thr <= n9               ICPFLOW_SIGHT_BEHIND 4   otherwise
 *   d_near_out float32 [n] or NULL: n9 (+inf for a row without a pixel).  d_counts int64 [6], required: the bad rows, then the
 *   rows of codes 0 .. 4, by ballot and popcount (integer atomics only).  n = 0 succeeds with six zeros.  Refusals as for the
 *   build (n for m), before any launch.
 *
 * icpflow_sight_segments -- the codes counted per segment of a labelled source cloud, BEFORE (q = d_before) and AFTER
 *   (q = d_after + d_flow; d_flow may be NULL, d_after may be d_before).  Segments are exactly icpflow_nn_residual_segments':
 *   the distinct values of d_labels float32 [n] ascending, -0.0 and +0.0 one label, a NaN label one segment per bit pattern;
 *   Lmax <= 4096; *d_num is the number of segments, or the NEGATIVE count when there are more (then no row of the table, no
 *   per-row code and nothing of d_info beyond zeros is written).
 *   d_d2_before, d_d2_after float32 [n] or NULL: what icpflow_nn_residual_segments writes per row.  A row is FAR iff its
 *   d2 > (float)far * (float)far (one fp32 product on the host); a miss holds r2, so it is far for any far <= r; 0 <= far <= 1e3.
 *   d_table double [Lmax][ICPFLOW_SIGHT_COLS], row c = the c-th label (rows from *d_num on are not written):
 *       0        label                                1        rows of the segment
 *       2        BEFORE: good rows                    3 - 12   BEFORE: for code k = 0 .. 4 column 3 + 2 k its rows, column
 *                                                              4 + 2 k the FAR rows among them (0 where d_d2_before is NULL)
 *       13       AFTER: good rows                     14 - 23  AFTER: the same ten
 *   d_code_before, d_code_after int32 [n] or NULL: the per-row codes, equal to what icpflow_sight_query writes.
 *   d_info int64 [12], required: icpflow_sight_query's d_counts of the BEFORE side, then of the AFTER side (the segments' counts
 *   add up to them exactly).
 *   By icpflow_nn_residual_segments' scheme with integer columns: chunks of 1024 rows of the stable order, a workgroup of 256
 *   threads per chunk, counts by ballot and popcount, the chunks added in ascending order by a final kernel (csrc/sight.hip).
 *   Refusals, all before any launch: a null required pointer, a negative size, Lmax < 1, far or the parameters outside their
 *   ranges, a struct_size mismatch are ICPFLOW_E_ARG; n > 2^29 or Lmax > 4096 are ICPFLOW_E_LIMIT; fewer workspace bytes than
 *   the query says are ICPFLOW_E_WORKSPACE before anything is written; a workspace that is not 16-byte aligned is ICPFLOW_E_ARG.
 *   n = 0 succeeds with *d_num = 0.  The workspace is the caller's: icpflow_sight_segments_workspace_bytes(n, Lmax) =
 *       a(8 n) + a(72 Lmax) + a(4 (Lmax + 1)) + a(88 chunks) + a(T)
 *   bytes, a(x) = x rounded up to a multiple of 256: the stable order, the segments' (label, count, start) rows, the first chunk
 *   of every segment, chunks = floor(n / 1024) + min(n, Lmax) + 1 partials of 2 x 11 ints, and
 *   T = icpflow_cluster_table_workspace_bytes(max(n, 1), Lmax); 0 for arguments the call refuses.  Nothing in it is read before
 *   it is written.  All three calls are asynchronous on `stream`, with no host synchronisation and no allocation.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_SIGHT_COLS 24
#define ICPFLOW_SIGHT_OUTSIDE 0
#define ICPFLOW_SIGHT_NO_RETURN 1
#define ICPFLOW_SIGHT_SEEN_THROUGH 2
#define ICPFLOW_SIGHT_AT_FIRST_RETURN 3
#define ICPFLOW_SIGHT_BEHIND 4
typedef struct icpflow_sight_params {
    size_t struct_size; /* sizeof(icpflow_sight_params_t) */
    int W;              /* columns of the image */
    int H;              /* rows of the image */
    double tan_lo;      /* tangent of the lowest elevation in view */
    double tan_hi;      /* tangent of the highest (exclusive) */
    double min_range;   /* metres */
    double max_range;   /* metres */
    double margin_abs;  /* metres */
    double margin_rel;  /* share of the range */
} icpflow_sight_params_t;
int icpflow_sight_default_params(icpflow_sight_params_t *params);
int icpflow_sight_build(const float *d_target, int m, const double *h_origin, const icpflow_sight_params_t *params,
                        uint32_t *d_image, int64_t *d_info, icpflow_stream_t stream);
int icpflow_sight_query(const uint32_t *d_image, const icpflow_sight_params_t *params, const double *h_origin,
                        const float *d_query, const float *d_flow, int n, int32_t *d_code_out, float *d_near_out,
                        int64_t *d_counts, icpflow_stream_t stream);
size_t icpflow_sight_segments_workspace_bytes(int n, int Lmax);
int icpflow_sight_segments(const uint32_t *d_image, const icpflow_sight_params_t *params, const double *h_origin,
                           const float *d_before, const float *d_after, const float *d_flow, const float *d_labels, int n,
                           const float *d_d2_before, const float *d_d2_after, double far, double *d_table, int Lmax,
                           int32_t *d_num, int32_t *d_code_before, int32_t *d_code_after, int64_t *d_info, void *d_ws,
                           size_t ws_bytes, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(i)  trust byte: the verdicts of 8(g) and 8(h) per source point, for flows saved as pseudo labels.  No counterpart in the
 * reference; KEEP below is a stated policy, not a metric of the reference (COVERAGE.md, named deviations).
 *
 * icpflow_flow_trust -- a pure function of tables and arrays that earlier calls left on the device:
 *   d_after float32 [n,3], d_flow float32 [n,3] or NULL, d_labels float32 [n]: icpflow_nn_residual_segments' arguments of
 *   the same names; d_resid_table double [Lmax][ICPFLOW_NNRS_COLS] and d_num: what that call wrote; d_d2_after float32 [n]: its
 *   per-row output; d_sight_table double [Lmax][ICPFLOW_SIGHT_COLS] and d_code_after int32 [n]: what icpflow_sight_segments
 *   wrote for the same cloud, or both NULL (n > 0: one without the other is ICPFLOW_E_ARG; codes without a table always);
 *   d_pair_rows float32 [P][pair_stride], column 0 the source label of a matched pair -- the layout icpflow_flow_rigid_rows
 *   reads (P = 0: may be NULL).
 *   Segment c < *d_num is row c of the tables, both in ascending label order.  Its bits:
 *     MATCHED   its label (column 0, a double) equals, by IEEE == on the widened value, column 0 of some pair row: -0.0
 *               matches +0.0, a NaN matches nothing; a label listed twice counts once.
 *     SKIPPED   its label equals (IEEE ==) (double)skip[0] or (double)skip[1].  FIT is then 0.
 *     LISTED    not SKIPPED, column 10 (AFTER good rows) is not zero and column 16 / column 10 > above, one fp64 division: a
 *               mean EQUAL to `above` is not listed, a segment without a good row is not listed (SegmentResidual.worst).
 *     FIT       0 when not listed.  Listed, with a sight table: far = the sum of columns 15, 17, 19, 21, 23 (the AFTER far rows
 *               of codes 0 .. 4, in that order, in fp64), seen = column 19, excused = columns 15 + 17 + 23 (codes 0, 1, 4);
 *               1 "seen through" iff seen > share * far; else 2 "lost from view" iff excused > share * far; else 3 "undecided"
 *               (one fp64 product; SegmentSight.annotate).  Listed, without a sight table: 3.
 *   Row i finds its segment by binary search on table.hip's key of its label (csrc/labelkey.hpp) among the keys of column 0
 *   narrowed to float: -0.0 and +0.0 are one label, a NaN label finds the segment with its bit pattern.  A SIGNALLING NaN is
 *   quieted first (bit 22 set), on both sides: the table's float64 column has quieted it already -- widening a float does --,
 *   so a signalling-NaN label finds the segment of its quiet form if there is one.
 *   A row is BAD by icpflow_nn_residual's rule, the same device function, applied to d_after + d_flow (one fp32 addition per
 *   coordinate; d_flow NULL: to d_after); NEAR iff d2_after <= far2, far2 = (float)far * (float)far, one fp32 product on the
 *   host (a NaN d2 is not near); every other good row is FAR.
 *   d_trust uint8 [n]:
 *       bits 0-2  ROW   0 not judged (a bad row); 1 NEAR; far rows by d_code_after: 2 seen through (code 2), 3 at the first
 *                       return (code 3), 4 behind (code 4), 5 no return (code 1), 6 outside (code 0); 7 far with no code
 *                       given (d_code_after NULL, or a value that is none of the five)
 *       bits 3-4  FIT of the row's segment             bit 5  MATCHED            bit 6  SKIPPED
 *       bit 7     KEEP: ROW is neither 0 nor 2, and FIT is 0 or 2
 *   A row whose label has no segment gets the whole byte 0; with *d_num <= 0 (overflow is reported as the negative count)
 *   every row does.  *d_num above Lmax is read as Lmax.
 *   d_segment uint8 [Lmax]: bits 3-6 of segment c, the other bits 0; bytes from *d_num on are not written.
 *   d_counts int64 [ICPFLOW_TRUST_COUNTS], by ballot and popcount (integer atomics only): [0..7] the rows WITH a segment per
 *   ROW class; [8..11] the judged (ROW != 0) rows of segments that are not SKIPPED, per FIT class; [12] the rows with bit 5,
 *   [13] with bit 6, [14] with bit 7; [15] the rows without a segment.  [0..7] and [15] add up to n.
 *   Two launches (csrc/trust.hip): one thread per segment, the pair labels through LDS in tiles of 1024; then a workgroup of
 *   256 threads per 1024 rows with the segments' keys and bytes in LDS.  Exactly d_trust[0, n), d_segment[0, *d_num) and the
 *   sixteen counts are written.  No workspace, no host synchronisation, no allocation; asynchronous on `stream`.
 *   icpflow_trust_params_t: above in [0, 1e3] (default 0.1, RESIDUAL_EDGES[1]), far in [0, 1e3] (default 0.1), share in [0, 1)
 *   (default 0.5), skip (defaults -1e8f, -1.0f: the ground and the unclustered rows, which no registration moved).
 *   Refusals, all before any launch: a null required pointer, a negative size, Lmax < 1, pair_stride < 1, P > 0 with no pair
 *   rows, a sight table without codes or codes without a sight table, a struct_size mismatch, above or far outside [0, 1e3]
 *   (a NaN too), share outside [0, 1) are ICPFLOW_E_ARG; n > 2^29 or Lmax > 4096 are ICPFLOW_E_LIMIT.  n = 0 succeeds with
 *   sixteen zeros.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_TRUST_COUNTS 16
typedef struct icpflow_trust_params {
    size_t struct_size; /* sizeof(icpflow_trust_params_t) */
    double above;       /* a segment is LISTED when its AFTER mean distance exceeds this; default 0.1 */
    double far;         /* a row is FAR when d2_after > (float)far * (float)far; default 0.1 */
    double share;       /* majority share of the verdict; default 0.5 */
    float skip[2];      /* labels no registration moved; default -1e8f, -1.0f */
} icpflow_trust_params_t;
int icpflow_flow_trust_default_params(icpflow_trust_params_t *params);
int icpflow_flow_trust(const float *d_after, const float *d_flow, const float *d_labels, int n, const double *d_resid_table,
                       const double *d_sight_table, const int32_t *d_num, int Lmax, const float *d_d2_after,
                       const int32_t *d_code_after, const float *d_pair_rows, int P, int pair_stride,
                       const icpflow_trust_params_t *params, uint8_t *d_trust, uint8_t *d_segment, int64_t *d_counts,
                       icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(j)  object boxes: an oriented box per segment and a box, a velocity and a heading per matched pair, for object pseudo
 * labels.  No counterpart in the reference; the fitting rule and the 0.5 m/s that tells movers from standing objects are
 * stated policies (COVERAGE.md, named deviations).
 *
 * icpflow_segment_boxes -- one box per segment of ONE labelled cloud:
 *   d_points float32 [n,3]; d_order int64 [n], d_table double [Lmax][9] and d_num: exactly what icpflow_cluster_table /
 *   icpflow_cluster_table_pair wrote for that cloud (its dictionary, stable order, counts and starts are reused, not rebuilt);
 *   h_dirs (HOST) float32 [A][2]: unit vectors (c_k, s_k), 1 <= A <= ICPFLOW_BOX_MAX_DIRECTIONS, copied before the call
 *   returns (they travel in the kernel arguments) -- the directions are the caller's, so no libm enters the contract;
 *   delta (metres) in [0, 1e3]; d_boxes double [Lmax][ICPFLOW_BOX_COLS].
 *   Arithmetic, float32, every fused operation an explicit fmaf: r = (float) of the table's centroid (columns 3, 4);
 *   x' = x - r_x, y' = y - r_y (one subtraction each: a cluster kilometres from the origin keeps its precision);
 *   u = fmaf(y', s_k, x' * c_k); v = fmaf(y', c_k, -(x' * s_k)).  A row is GOOD iff its three coordinates are finite; the
 *   other rows enter nothing (the centroid is the table's, though: a segment that holds such rows has a centroid that is not
 *   finite, and its box is then NaN, with its good rows counted).  Per direction k over the good rows: umin, umax, vmin, vmax; area = (umax - umin) * (vmax - vmin)
 *   in float32; near = the rows with min(min(umax - u, u - umin), min(vmax - v, v - vmin)) <= (float)delta, float32
 *   subtractions of the same u and v the extrema were taken from.  The best k maximises near, then minimises area, then k.
 *   Row c < *d_num of d_boxes:
 *       0  label            1  rows (the table's count)    2  good rows        3  k           4  near at k
 *       5  area at k, widened                              6-8  the centre, in fp64 in this order and without fma:
 *            um = ((double)umin + (double)umax) * 0.5, vm likewise; X = (double)r_x + ((double)c_k * um - (double)s_k * vm);
 *            Y = (double)r_y + ((double)s_k * um + (double)c_k * vm); Z = ((double)zmin + (double)zmax) * 0.5
 *       9  du = (double)umax - (double)umin    10  dv    11  height = (double)zmax - (double)zmin
 *       12-13  c_k, s_k widened                14-15  zmin, zmax
 *   A segment with a negative label (ground -1e8, noise -1: the cluster table computes no statistics for them either) and a
 *   segment without a good row get columns 0 and 1, column 3 = -1 and zeros elsewhere.  Rows from *d_num on are not written;
 *   with *d_num <= 0 (overflow is reported as the negative count) nothing is; *d_num above Lmax is read as Lmax.
 *   What the table claims is clipped to the cloud and never dereferenced beyond it: a start outside [0, n] leaves its segment
 *   no row, a count is cut at n - start, an entry of d_order outside [0, n) is skipped.
 *   Workspace, the caller's, 16-byte aligned: icpflow_segment_boxes_workspace_bytes(n, Lmax, A) =
 *       a256(4 (Lmax + 1)) + a256(16 C A) + a256(8 C) + a256(4 C) + a256(16 Lmax A) + a256(8 Lmax) + a256(4 Lmax) + a256(4 Lmax A),
 *   C = n / 1024 + min(n, Lmax) + 1 chunks of 1024 rows, a256 = rounded up to a multiple of 256; non-decreasing in n, Lmax and
 *   A; 0 for arguments the call refuses.  Nothing in it is read before it is written.
 *   Five launches (csrc/boxes.hip), asynchronous on `stream`, no host synchronisation, no allocation, no floating-point atomic:
 *   every number is a function of the arguments alone.
 *   Refusals, all before any launch: a null required pointer, n < 0, Lmax < 1, A outside [1, 360], delta outside [0, 1e3] (a NaN
 *   too), a direction that is not finite or has |c * c + s * s - 1| > 1e-3 (in fp64), a workspace not 16-byte aligned are
 *   ICPFLOW_E_ARG; n > 2^29 or Lmax > 4096 are ICPFLOW_E_LIMIT; a missing or short workspace is ICPFLOW_E_WORKSPACE.  n = 0
 *   succeeds (every segment of the table is then without a row).
 *
 * icpflow_pair_objects -- one row per matched pair, from the two box tables and what the registration left on the device:
 *   d_boxes_src, d_num_src: icpflow_segment_boxes' table of the source cloud; d_boxes_dst, d_num_dst: of the destination, or
 *   both NULL; d_pair_rows float32 [P][pair_stride], pair_stride >= 2: column 0 the source label, column 1 the destination
 *   label of a pair; d_T float32 [P][16], row-major 4 x 4; d_objects double [P][ICPFLOW_OBJECT_COLS]; d_counts int64
 *   [ICPFLOW_OBJECT_COUNTS].  A label finds its segment as icpflow_flow_trust's rows do: by binary search on the key
 *   (csrc/labelkey.hpp) of the quieted label among column 0 narrowed to float.  A segment HAS A BOX iff its column 3 >= 0.
 *   Row p, everything in fp64 in the order written, no fma:
 *       0-1    the two labels                      2-3    their segments' indices, or -1
 *       4-6    c = the source box's centre         7-9    d = T c - c: d_x = (((m00 cx + m01 cy) + m02 cz) + m03) - cx, ...
 *       10-12  d / seconds                         13     vx vx + vy vy (the square root is the caller's)
 *       14     moving: 1 iff column 13 >= min_speed * min_speed (one product on the host)
 *       15     the heading's quadrant m among e0 = (c_k, s_k), e1 = (-s_k, c_k), e2 = -e0, e3 = -e1 -- moving: the m with the
 *              largest e_m . d_xy (ex dx + ey dy), ties to the lowest m; standing: 0 if du >= dv, else 1
 *       16-18  length (the extent along e_m), width, height                    19-20  e_m
 *       21     the squared xy distance of c + d from the destination box's centre; -1 without a destination box
 *       22-23  the good rows of the source and of the destination box (0 without one)
 *   A pair whose source segment is missing or has no box gets columns 0-3 and zeros elsewhere.
 *   d_counts: [0] pairs with a source box, [1] of them moving, [2] pairs whose source label finds no segment, [3] pairs whose
 *   destination label finds none (every pair when there is no destination table); by ballot and popcount, integer atomics only.
 *   One launch, one thread per pair, no workspace; asynchronous on `stream`.  Refusals, before any launch: a null required
 *   pointer, P < 0, Lmax < 1, pair_stride < 2, one of the destination's two arguments without the other, P > 0 with no pair
 *   rows or no transforms, a struct_size mismatch, seconds not positive and finite, min_speed negative or not finite are
 *   ICPFLOW_E_ARG; Lmax > 4096 is ICPFLOW_E_LIMIT.  P = 0 succeeds with four zeros.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_BOX_COLS 16
#define ICPFLOW_BOX_MAX_DIRECTIONS 360
#define ICPFLOW_OBJECT_COLS 24
#define ICPFLOW_OBJECT_COUNTS 4
typedef struct icpflow_object_params {
    size_t struct_size; /* sizeof(icpflow_object_params_t) */
    double seconds;     /* the time between the two sweeps; default 0.1 */
    double min_speed;   /* an object moves when its xy speed reaches this, m/s; default 0.5 */
} icpflow_object_params_t;
size_t icpflow_segment_boxes_workspace_bytes(int n, int Lmax, int A);
int icpflow_segment_boxes(const float *d_points, int n, const int64_t *d_order, const double *d_table, const int32_t *d_num,
                          int Lmax, const float *h_dirs, int A, double delta, double *d_boxes, void *d_ws, size_t ws_bytes,
                          icpflow_stream_t stream);
int icpflow_pair_objects_default_params(icpflow_object_params_t *params);
int icpflow_pair_objects(const double *d_boxes_src, const int32_t *d_num_src, const double *d_boxes_dst,
                         const int32_t *d_num_dst, int Lmax, const float *d_pair_rows, int P, int pair_stride, const float *d_T,
                         const icpflow_object_params_t *params, double *d_objects, int64_t *d_counts, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(k)  object tracks: the clusters of ONE sweep under several labellings linked into tracks, and a constant velocity fitted
 * per track over all the gaps of a multi-frame sample (every frame pair of a sample ends at frame 0: the destination sweep
 * is shared, row for row, and every gap re-clusters it).  No counterpart in the reference; the linking rule, min_iou 0.5,
 * max_residual 0.2 m and min_speed 0.5 m/s are stated policies (COVERAGE.md, named deviations).
 *
 * icpflow_label_overlap -- which segments of two labellings of the same n rows are the same set of rows:
 *   d_labels_a, d_labels_b float32 [n]; d_table_a, d_table_b double [Lmax][ICPFLOW_OVERLAP_COLS]; d_num_a, d_num_b int32 [1];
 *   d_counts int64 [ICPFLOW_OVERLAP_COUNTS].  Segments are the distinct labels in ascending order, as icpflow_cluster_table
 *   reports them (+0.0 and -0.0 one label, reported as 0.0; NaNs kept apart by their bits, behind +inf or, with the sign bit, before -inf).  A label < 0 (ground
 *   -1e8, noise -1, -inf) is NO SEGMENT TO LINK: its rows enter no intersection and its segment gets no partner; every other
 *   label, a NaN too, is.  inter(c, e) = the rows in segment c of one side and segment e of the other, both linkable.
 *   The PARTNER of c is the e with the largest inter(c, e) > 0, ties to the lower e (the ascending label order).
 *   Row c < *d_num_a of d_table_a (d_table_b likewise, the roles exchanged):
 *       0  label                      1  rows of the segment         2  of them, rows whose other label is linkable
 *       3  partner e, or -1           4  its label (0 without one)   5  inter(c, partner)
 *       6  the second-largest inter(c, .), the partner's left out (0 without one; equal to column 5 on a tie)
 *       7  the partner's rows         8  mutual: 1 iff the partner's own partner is c
 *       9  IoU = col 5 / (col 1 + col 7 - col 5): ONE fp64 division of exact integers; 0 without a partner
 *   d_counts: [0] rows linkable on both sides, [1] mutual pairs (each has IoU > 0), [2] segments of A with a partner, [3] of B.
 *   *d_num_a, *d_num_b: the segments of each side, or the negative count when a side holds more than Lmax labels (as
 *   icpflow_cluster_table); if either is negative NEITHER table is written and d_counts is four zeros.  Rows from *d_num on are
 *   not written.  n = 0 succeeds with both numbers 0 and four zeros.
 *   Every number is an exact integer count or one fp64 division of such counts; integer atomics in LDS only, no
 *   floating-point atomic: the output is a function of the arguments alone, whatever the stream and the scheduling.
 *   Workspace, the caller's, 16-byte aligned: icpflow_label_overlap_workspace_bytes(n, Lmax), a multiple of 256, non-decreasing
 *   in n and Lmax, 0 for arguments the call refuses; nothing in it is read before it is written.  Asynchronous on `stream`, no
 *   host synchronisation, no allocation (csrc/overlap.hip: segments cut into chunks of 1024 rows, a workgroup per chunk, the
 *   other side's segment indices counted in an LDS histogram of Lmax integers; a workgroup per segment folds its chunks).
 *   Refusals, all before any launch: a null required pointer, n < 0, Lmax < 1, a workspace not 16-byte aligned are
 *   ICPFLOW_E_ARG; n > 2^29 or Lmax > 4096 are ICPFLOW_E_LIMIT; a missing or short workspace is ICPFLOW_E_WORKSPACE.
 *
 * icpflow_object_tracks_extend -- one gap of a sample: the track ids of the shared sweep's rows carried on.
 *   State, the caller's, on the device: d_track_of_row int32 [n] (-1 = no track; all -1 before the first gap) and d_next_id
 *   int32 [1] (0 before the first gap).  d_labels float32 [n]: this gap's labels of the shared sweep.  They are overlapped
 *   (icpflow_label_overlap's kernels) with the labelling "track id per row" -- an id is its own label, -1 is negative.
 *   A linkable segment INHERITS the id of its partner iff mutual and IoU >= min_iou (so linking is one to one); every other
 *   linkable segment is FRESH and takes *d_next_id + its rank among the fresh segments in ascending label order.  The rows of
 *   every linkable segment are set to its id, the other rows keep theirs; *d_next_id advances by the fresh segments.
 *   d_segments double [Lmax][ICPFLOW_TRACK_SEGMENT_COLS], row c < *d_num:
 *       0  label    1  rows    2  track id (-1: not linkable)    3  inherited    4  inter with its partner    5  IoU
 *   (columns 4 and 5 are the overlap's whether or not the link was taken; 0 without a partner).
 *   d_objects double [P][ICPFLOW_OBJECT_COLS]: this gap's table of icpflow_pair_objects, or NULL with P = 0; d_obs double
 *   [P][ICPFLOW_TRACK_OBS_COLS], row p:
 *       0  the track id of the pair's destination label (column 1 of the object row; its segment found by binary search on the
 *          key of the quieted label, as icpflow_pair_objects does), or -1 when the pair has no box (its column 22 is not
 *          positive) or the label finds no linkable segment
 *       1  gap    2  seconds    3-5  the displacement (columns 7-9)    6  max(length, width)    7  min(length, width)
 *       8  height    9  source points (column 22)    10-12  the centre (columns 4-6)
 *   d_counts int64 [ICPFLOW_TRACK_EXTEND_COUNTS]: segments (linkable), inherited, fresh, observations with an id, observations
 *   without, overflow.  OVERFLOW: more than Lmax distinct labels, more than Lmax distinct values in d_track_of_row (the live
 *   ids and -1), or an id beyond 2^24 (ids travel as float32 labels): overflow = 1, *d_num is negative, d_track_of_row and *d_next_id keep every bit, d_segments is
 *   not written, every row of d_obs has id -1.
 *   gap in [0, 63]; seconds positive and finite: the time this gap spans.  params: icpflow_track_params_t from
 *   icpflow_object_tracks_default_params (min_iou 0.5 in (0, 1], max_residual 0.2 m, min_speed 0.5 m/s; for min_iou > 0.5
 *   mutuality is implied).  Workspace: icpflow_object_tracks_extend_workspace_bytes(n, Lmax), as above.  Asynchronous on
 *   `stream`; fresh ids come from a scan, never from the order in which workgroups finish.
 *   Refusals, before any launch: a null required pointer (d_objects with P > 0, d_obs with P > 0), n < 0, P < 0, Lmax < 1, gap
 *   outside [0, 63], seconds not positive and finite, a struct_size mismatch, min_iou outside (0, 1], a negative or
 *   non-finite max_residual or min_speed, a misaligned workspace are ICPFLOW_E_ARG; n > 2^29 or Lmax > 4096 are
 *   ICPFLOW_E_LIMIT; a short workspace is ICPFLOW_E_WORKSPACE.
 *
 * icpflow_object_tracks_fit -- one row per track from the observations of all gaps:
 *   d_obs double [M][ICPFLOW_TRACK_OBS_COLS], the gaps concatenated in gap order; T: the tracks (ids 0 .. T - 1, T = *d_next_id
 *   read by the caller or an upper bound); d_tracks double [T][ICPFLOW_TRACK_COLS]; d_counts int64 [ICPFLOW_TRACK_FIT_COUNTS].
 *   One thread per track walks the M rows in ascending order, fp64, every operation written out, no fma; with s = seconds and
 *   d the displacement of an observation of the track:
 *       0  id    1  observations    2  the bit mask of the gaps seen, as a double    3-5  v = (sum s d) / (sum s s) per axis
 *       6  sqrt(vx vx + vy vy)     7  sqrt of the largest r2 = (dx - s vx)^2 + (dy - s vy)^2     8  sqrt((sum r2) / observations)
 *       9  moving: observed and col 6 >= min_speed    10  judged: seen in at least two distinct gaps (gaps outside [0, 63] set no bit)
 *       11  consistent: judged and col 7 <= max_residual
 *       12-14  the largest long side, short side and height over the views    15  the most source points in one view
 *   A track without an observation has its id and zeros.  All pairs of a sample end at frame 0: constant velocity means
 *   d_j = s_j v, least squares through the origin.  d_counts: tracks, observed (>= 1 observation), judged, consistent, moving
 *   (observed and col 9).  Refusals: a null required pointer, M < 0, T < 0, a struct_size mismatch, parameters as above are
 *   ICPFLOW_E_ARG; M or T > 2^24 is ICPFLOW_E_LIMIT.  T = 0 succeeds with five zeros.  No workspace.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_OVERLAP_COLS 10
#define ICPFLOW_OVERLAP_COUNTS 4
#define ICPFLOW_TRACK_SEGMENT_COLS 6
#define ICPFLOW_TRACK_OBS_COLS 13
#define ICPFLOW_TRACK_COLS 16
#define ICPFLOW_TRACK_EXTEND_COUNTS 6
#define ICPFLOW_TRACK_FIT_COUNTS 5
typedef struct icpflow_track_params {
    size_t struct_size;  /* sizeof(icpflow_track_params_t) */
    double min_iou;      /* a segment inherits a track at this IoU or more; default 0.5 */
    double max_residual; /* metres: a track is consistent when no observation lies farther from the fitted line; default 0.2 */
    double min_speed;    /* a track moves when its fitted xy speed reaches this, m/s; default 0.5 */
} icpflow_track_params_t;
size_t icpflow_label_overlap_workspace_bytes(int n, int Lmax);
int icpflow_label_overlap(const float *d_labels_a, const float *d_labels_b, int n, int Lmax, double *d_table_a, int32_t *d_num_a,
                          double *d_table_b, int32_t *d_num_b, int64_t *d_counts, void *d_ws, size_t ws_bytes,
                          icpflow_stream_t stream);
int icpflow_object_tracks_default_params(icpflow_track_params_t *params);
size_t icpflow_object_tracks_extend_workspace_bytes(int n, int Lmax);
int icpflow_object_tracks_extend(const float *d_labels, int n, int Lmax, int32_t *d_track_of_row, int32_t *d_next_id,
                                 const double *d_objects, int P, int gap, double seconds, const icpflow_track_params_t *params,
                                 double *d_segments, int32_t *d_num, double *d_obs, int64_t *d_counts, void *d_ws, size_t ws_bytes,
                                 icpflow_stream_t stream);
int icpflow_object_tracks_fit(const double *d_obs, int M, int T, const icpflow_track_params_t *params, double *d_tracks,
                              int64_t *d_counts, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(l)  object tracks across the files of a log: ids carried by nearest rows.  Consecutive frame-pair files of a log share a
 * sweep -- the destination of file k is the source of file k + 1 -- but not its rows: the two views differ in order, crop and
 * ground removal, and in the float32 rounding of the pose product.  Row identity (8(k)) is replaced by "the nearest row
 * within a small radius after applying the pose".  No counterpart in the reference; the radius, min_share, max_dv and
 * min_speed are stated policies (COVERAGE.md, named deviations).
 *
 * icpflow_rows_carry -- an id per row of one view from the ids of the other view's rows.
 *   d_prev float32 [m,3] and d_prev_id int32 [m]: one view of a sweep and an id per row, a negative id means none; h_pose
 *   double [16], row-major 4 x 4, HOST: it maps d_prev's coordinates into d_next's; d_next float32 [n,3]: the other view;
 *   radius in [1e-3, 1e3] metres; min_share in [0, 1].
 *   Arithmetic: the pose is narrowed to float on the host; a previous row is moved in fp32 by
 *       x' = ((m00 x + m01 y) + m02 z) + m03,   y' and z' alike with rows 1 and 2,
 *   every operation rounded by itself.  After that every word of icpflow_nn_residual's contract (8(g)) holds with the moved
 *   previous rows as targets and d_next as queries without a flow: r2 = (float)r * (float)r, d2 = (dx dx + dy dy) + dz dz, a
 *   hit iff d2 <= r2, the LOWEST previous row on equal d2, the same grid and the same exact search.  Bad rows: a query with a
 *   non-finite coordinate or one beyond +-1e6 m; a previous row with such a coordinate BEFORE OR AFTER the move (a pad row
 *   (1e8, 1e8, 1e8) stays bad under a rotation that happens to cancel it) -- it is never a neighbour.
 *   d_id int32 [n]: the id of the hit's previous row; -1 without a hit, for a bad query, or where that row's id is negative.
 *   d_d2 float32 [n] and d_idx int32 [n], each may be NULL: as icpflow_nn_residual defines d_d2_out and d_idx_out (no hit:
 *   r2 and -1, a bad query: r2 and -2).
 *   d_counts int64 [ICPFLOW_CARRY_COUNTS]: [0] queries with a hit, [1] of them those whose previous row has an id >= 0,
 *   [2] misses, [3] bad queries, [4] bad previous rows, [5] BROKEN.  BROKEN is decided on the device by a closing launch:
 *   1 iff (double)counts[0] < min_share * (double)n, one fp64 product.  Every d_id is then -1 -- the chain starts afresh and no
 *   host sees a number in between --; d_d2, d_idx and counts [0] .. [4] are what they are without the break.  n = 0 is not
 *   broken; m = 0 with n > 0 is broken unless min_share is 0.
 *   Counts by ballot and popcount with integer atomics only; no floating-point atomic: every output is a function of the
 *   arguments alone.  Workspace, the caller's, 16-byte aligned: icpflow_rows_carry_workspace_bytes(n, m) =
 *   table(m) + table(n) + 2 a(4 n) with 8(g)'s table(k) and a(x): a multiple of 256, non-decreasing, 0 for sizes the call
 *   refuses; nothing in it is read before it is written.  Asynchronous on `stream`, no host synchronisation, no allocation.
 *   Refusals, all before any launch: a null required pointer (d_prev and d_prev_id with m > 0, d_next and d_id with n > 0,
 *   h_pose, d_counts), n < 0, m < 0, a radius or min_share outside its range, a pose entry that is not finite (as a float
 *   too), a misaligned workspace are ICPFLOW_E_ARG; n or m > 2^29 is ICPFLOW_E_LIMIT; a missing or short workspace is
 *   ICPFLOW_E_WORKSPACE.
 *
 * icpflow_pair_row_ids -- an id per row of one side of a frame pair, from the ids of its pairs.
 *   d_labels float32 [n]: the labels of that side's rows; d_pair_rows float32 [P][pair_stride] (pair_stride >= 2): column 0 the
 *   source label of a pair, column 1 its destination label; col: 0 for the source side, 1 for the destination side;
 *   d_pair_id int32 [P]; d_weight double, P values weight_stride doubles apart (column 22 of the object rows with stride
 *   ICPFLOW_OBJECT_COLS), or NULL: every pair weighs the same.
 *   A row takes the id of the pair whose label in column `col` equals its own: equality by the key of csrc/labelkey.hpp on
 *   the quieted label, as icpflow_flow_trust finds MATCHED by keys (+0.0 and -0.0 one label, NaNs by their bits).  Among
 *   several such pairs with an id >= 0 the largest weight wins (a NaN weighs least); on a tie, or without weights, the
 *   lowest p.  A row gets -1 when its label is negative, has no such pair, or has only pairs with negative ids.
 *   d_row_id int32 [n]; d_counts int64 [ICPFLOW_PAIR_ROW_ID_COUNTS]: [0] rows with an id, [1] rows without, [2] pairs whose
 *   label (column col) an earlier pair has too.
 *   Two launches: a thread per pair builds a table of (key, winner) sorted by key -- the pairs pass through LDS in tiles of
 *   1024, a pair's slot is its rank --, then a workgroup of 256 threads per 1024 rows finds each row's key by binary search.
 *   Workspace: icpflow_pair_row_ids_workspace_bytes(P) (a multiple of 256, constant in P, 0 for a P the call refuses),
 *   16-byte aligned.  Refusals before any launch: a null required pointer, n < 0, P < 0, col outside {0, 1}, pair_stride < 2,
 *   weight_stride < 1 with weights, a misaligned workspace are ICPFLOW_E_ARG; n > 2^29 or P > ICPFLOW_PAIR_ROW_ID_MAX_PAIRS are
 *   ICPFLOW_E_LIMIT; a missing or short workspace is ICPFLOW_E_WORKSPACE.
 *
 * icpflow_object_tracks_extend_side -- icpflow_object_tracks_extend (8(k)) with one more argument, `side`.  With side 1 it IS
 *   that call, bit for bit.  With side 0 d_labels are the SOURCE labels of the file, d_track_of_row has n = source rows, and
 *   column 0 of an observation is found through the pair's SOURCE label (column 0 of the object row; "has a box" is still
 *   column 22 > 0).  Everything else is word for word the same: overlap, inherit or fresh, ids by a scan in label order,
 *   overflow.  side outside {0, 1} is ICPFLOW_E_ARG; the workspace is icpflow_object_tracks_extend_workspace_bytes(n, Lmax).
 *
 * icpflow_object_tracks_path -- one row per track over a log.
 *   d_obs double [M][ICPFLOW_TRACK_OBS_COLS]: the files' observation tables concatenated in file order; d_step int32 [M]: the
 *   file index of each observation, from 0, non-decreasing; d_frames double [F][12]: per file the rotation (9 values,
 *   row-major) and the translation that map that file's destination frame into the log's frame (the host forms the chain in
 *   fp64: W_0 = I, W_{k+1} = W_k inverse(pose_{k+1}), the inverse of a rigid pose (R, t) being (R^T, -R^T t)); T: the tracks
 *   (ids 0 .. T - 1).  d_paths double [T][ICPFLOW_TRACK_PATH_COLS]; d_counts int64 [ICPFLOW_TRACK_PATH_COUNTS].
 *   One thread per track walks the M rows in ascending order; fp64, every operation written out, no fma.  An observation with
 *   a step outside [0, F) is left out.  Of the observations of one track in one step -- consecutive rows of the track with
 *   the same step -- the one with the most source points (column 9) COUNTS, the lower row on a tie.  Per counted
 *   observation with centre c, displacement d, seconds s and its step's (R, t):
 *       c_w = R c + t: ((R00 cx + R01 cy) + R02 cz) + tx, ...;   d_w = R d: (R00 dx + R01 dy) + R02 dz, ...;   v = d_w / s
 *   Row t:
 *       0  id    1  counted observations    2  first step    3  last step    4  steps missing in between: (last - first + 1) - col 1
 *       5  the sum of s    6  path length, the sum of sqrt(dwx dwx + dwy dwy)    7-9  mean velocity, (sum of d_w) / col 5
 *       10  sqrt(vx vx + vy vy) of it
 *       11  the largest sqrt((vx' - vx)^2 + (vy' - vy)^2) over counted observations at ADJACENT steps s, s + 1; 0 without one
 *       12  the number of such pairs
 *       13  jump: the largest xy distance of c_w + d_w at step s from c_w at step s + 1 over the same pairs; reported, no verdict
 *           hangs on it
 *       14  moving: col 1 > 0 and col 10 >= min_speed    15  judged: col 12 >= 1    16  smooth: judged and col 11 <= max_dv
 *       17-19  the largest long side, short side and height over the counted views    20  the most source points in one view
 *       21-23  c_w of the first counted observation
 *   A track without a counted observation has its id and zeros.  d_counts: tracks, observed, judged, smooth, moving.
 *   params: icpflow_track_path_params_t from icpflow_object_tracks_path_default_params (max_dv 1.0 m/s: a velocity change
 *   of 10 cm per 0.1 s sweep -- a log-long track cannot be held to one constant velocity, cars brake; min_speed 0.5 m/s).
 *   Refusals: a null required pointer (d_obs and d_step with M > 0, d_frames with F > 0, d_paths with T > 0, params,
 *   d_counts), a negative size, F < 1 with M > 0, a struct_size mismatch, a negative or non-finite parameter are
 *   ICPFLOW_E_ARG; M, T or F > 2^24 is ICPFLOW_E_LIMIT.  T = 0 succeeds with five zeros.  No workspace.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_CARRY_COUNTS 6
#define ICPFLOW_PAIR_ROW_ID_COUNTS 3
#define ICPFLOW_PAIR_ROW_ID_MAX_PAIRS 4096
#define ICPFLOW_TRACK_PATH_COLS 24
#define ICPFLOW_TRACK_PATH_COUNTS 5
typedef struct icpflow_track_path_params {
    size_t struct_size; /* sizeof(icpflow_track_path_params_t) */
    double max_dv;      /* m/s: a track is smooth when its velocity changes by no more between adjacent steps; default 1.0 */
    double min_speed;   /* a track moves when its mean xy speed reaches this, m/s; default 0.5 */
} icpflow_track_path_params_t;
size_t icpflow_rows_carry_workspace_bytes(int n, int m);
int icpflow_rows_carry(const float *d_prev, const int32_t *d_prev_id, int m, const double *h_pose, const float *d_next, int n,
                       double radius, double min_share, int32_t *d_id, float *d_d2, int32_t *d_idx, int64_t *d_counts, void *d_ws,
                       size_t ws_bytes, icpflow_stream_t stream);
size_t icpflow_pair_row_ids_workspace_bytes(int P);
int icpflow_pair_row_ids(const float *d_labels, int n, const float *d_pair_rows, int P, int pair_stride, int col,
                         const int32_t *d_pair_id, const double *d_weight, int weight_stride, int32_t *d_row_id, int64_t *d_counts,
                         void *d_ws, size_t ws_bytes, icpflow_stream_t stream);
int icpflow_object_tracks_extend_side(const float *d_labels, int n, int Lmax, int32_t *d_track_of_row, int32_t *d_next_id,
                                      const double *d_objects, int P, int side, int gap, double seconds,
                                      const icpflow_track_params_t *params, double *d_segments, int32_t *d_num, double *d_obs,
                                      int64_t *d_counts, void *d_ws, size_t ws_bytes, icpflow_stream_t stream);
int icpflow_object_tracks_path_default_params(icpflow_track_path_params_t *params);
int icpflow_object_tracks_path(const double *d_obs, const int32_t *d_step, int M, const double *d_frames, int F, int T,
                               const icpflow_track_path_params_t *params, double *d_paths, int64_t *d_counts,
                               icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(m)  track repair: the gap that breaks a track's constant velocity registered again from the motion the other gaps predict.
 * 8(k) ends in a verdict -- a track is not consistent --; here the observation that breaks it is named, its pair is registered
 * once more from the predicted displacement, and the new pose replaces the old one only where the data prefer it.  Multi-frame
 * samples only (all gaps share the destination sweep).  No counterpart in the reference; which gap is retried, the acceptance
 * rule and its numbers are stated policies (COVERAGE.md, named deviations).  The partner of a pair is not chosen again; a gap
 * without a pair is filled by 8(n).
 *
 * icpflow_object_tracks_suspects -- which observation breaks its track:
 *   d_obs double [M][ICPFLOW_TRACK_OBS_COLS], the gaps concatenated as icpflow_object_tracks_fit takes them; T: the tracks;
 *   params: icpflow_track_params_t, of which only max_residual is read; d_plan double [M][ICPFLOW_TRACK_PLAN_COLS]; d_counts
 *   int64 [ICPFLOW_TRACK_PLAN_COUNTS].  One thread per observation j walks the M rows in ascending order, twice, fp64, every
 *   operation written out, no fma.  Observation j HAS AN ID iff its column 0, t, has 0 <= t < T (a NaN has none); without one
 *   its plan row is zeros.  First walk, over the rows i != j whose column 0 equals t, with s = seconds and d the displacement:
 *   A += s_i s_i; B += s_i d_i per axis; the bit of gap_i is set for a gap in [0, 63]; others += 1.  j is ELIGIBLE iff at least
 *   two distinct gaps were seen and A > 0; then v = B / A per axis.  Second walk, over the same rows:
 *   inner = the largest (dx_i - s_i vx)^2 + (dy_i - s_i vy)^2.  With p = s_j v, r2 = (dx_j - p_x)^2 + (dy_j - p_y)^2 and
 *   m2 = max_residual * max_residual (one product), j is SUSPECT iff eligible, inner <= m2 and r2 > m2: the other gaps agree
 *   among themselves on one velocity, and this gap does not agree with it.  Row j of d_plan:
 *       0  suspect    1  others    2  the distinct gaps among the others    3-5  p    6  sqrt(r2)    7  sqrt(inner)
 *   (columns 0 and 3-7 are zero for a row that is not eligible).  d_counts: rows with an id, eligible rows, eligible rows with
 *   inner <= m2, suspects; by ballot and popcount, integer atomics only.  One launch, no workspace, asynchronous on `stream`.
 *   Refusals, before any launch: a null required pointer (d_obs and d_plan with M > 0, params, d_counts), M < 0, T < 0, a
 *   struct_size mismatch, a negative or non-finite max_residual are ICPFLOW_E_ARG; M > 2^16 (the walk is quadratic) or
 *   T > 2^24 is ICPFLOW_E_LIMIT.  M = 0 succeeds with four zeros.
 *
 * icpflow_pairs_repair_select -- does the new pose replace the old one; one thread per retried pair, one launch, no workspace:
 *   d_T_new, d_T_old float32 [K][16], row-major 4 x 4; d_iters int32 [1]: the iteration count of the ICP batch that made
 *   d_T_new, negative when the batch was abandoned; d_errors, d_ious float32 [K][2], d_translations, d_rotations float32
 *   [K][3]: the metrics of the new pose as icpflow_match_eval leaves them; d_errors_old float32 [K][2]: the errors of the old
 *   pose on the same clouds; d_centre double [K][3]: columns 4-6 of the pair's row of icpflow_pair_objects; d_pred double
 *   [K][3]: columns 3-5 of its plan row.  params: icpflow_repair_params_t, its defaults (icpflow_pairs_repair_default_params) 2.0, 0.2,
 *   9.0, 0.2, 0.2; the four thresholds of the association are narrowed to float32 and compared as the association compares them.
 *   e = min(error_src, error_dst) in float32, NaN if either is (e_new of d_errors, e_old of d_errors_old).
 *   d = T_new c - c in fp64 in the order of icpflow_pair_objects' columns 7-9.  The REASON is the first test that fails:
 *       5  *d_iters < 0: the batch was abandoned
 *       1  the association's reject test on the new pose (icpflow_assoc_assign: translation norm, min(iou) by the reference's
 *          rule, the two angles; the same device code, csrc/rejecttest.hpp) fails
 *       2  e_new is NaN or not < thres_error
 *       3  (d_x - p_x)^2 + (d_y - p_y)^2 > max_residual * max_residual: the new pose is not where the track predicts
 *       4  e_new > e_old, a NaN e_old read as +inf (a new pose with an error replaces an old one without): the data must
 *          prefer the new pose -- an object that really left its line is not slid back onto it; e_new == e_old accepts
 *       0  otherwise: accepted
 *   d_T_out float32 [K][16]: T_new when accepted, T_old bit for bit otherwise.  d_report double [K][ICPFLOW_REPAIR_COLS]:
 *       0  reason    1  e_new    2  e_old    3-5  d    6  the xy distance of d from p    7  *d_iters    8  min(iou)
 *       9  the translation norm    10  fmaxf of the two tested angles' magnitudes    11  accepted
 *   (every column is written whatever the reason).  d_counts int64 [ICPFLOW_REPAIR_COUNTS]: one count per reason 0 to 5, then
 *   two zeros (word 6 is the caller's: pairs it did not retry).  Refusals, before any launch: a null required pointer, K < 0, a
 *   struct_size mismatch, a negative or non-finite parameter are ICPFLOW_E_ARG; K > 2^24 is ICPFLOW_E_LIMIT.  K = 0 succeeds
 *   with eight zeros.
 *
 * icpflow_pairs_reregister -- K pairs of one frame pair registered again, everything enqueued on `stream`, no host
 *   synchronisation, no allocation:  tables: both clouds as icpflow_cluster_table leaves them (d_table_*, S, D and
 *   label_stride are not read); d_seg int64 [2,3,K]: the segment rows of icpflow_gather_segments, source cloud first, every
 *   length <= N and every offset -1 (no subsample: a cluster longer than N is the caller's to leave out); d_clouds float32
 *   [2,K,N,4]: scratch for the padded batch; d_init float32 [K][16]; d_T_old, d_centre, d_pred as above; reg: thres_dist,
 *   relative_rmse_thr, max_iterations and stop_mode are read, the edges are not.  In this order:
 *   icpflow_gather_segments of both sides; icpflow_apply_icp, source onto destination from d_init (unlike icpflow_hist_icp
 *   there is no swap by length); icpflow_match_eval of T_new; icpflow_match_eval of T_old (source, destination, as
 *   icpflow_register_stage orders them); the select.  T_new and both sets of metrics are, bit for bit, what those entry points
 *   give on the gathered batch.  d_T_out, d_report, d_counts: the select's.
 *   Workspace, the caller's, 16-byte aligned: icpflow_pairs_reregister_workspace_bytes(K, N) =
 *       a256(4 (44 K + 1)) + a256(icpflow_workspace_bytes(K, N, 0, 0, 0)),
 *   a multiple of 256, non-decreasing in K and N, 0 for sizes the call refuses (and for K = 0, which needs none); nothing in
 *   it is read before it is written.  Its first region holds, after the call, float32 [T_new 16K | errors 2K | inliers 2K |
 *   ratios 2K | ious 2K | translations 3K | rotations 3K | the same six arrays of T_old, 14K | the iteration count (int32)].
 *   Refusals, before any launch: a null required pointer, K < 0, N < 1, max_iterations outside [1, 1024], an unknown stop_mode,
 *   a negative or non-finite thres_dist, the parameter block as above, a misaligned workspace are ICPFLOW_E_ARG; K N > 2^30 is
 *   ICPFLOW_E_LIMIT; a missing or short workspace is ICPFLOW_E_WORKSPACE.  An options block the cores refuse is refused by
 *   them, behind the gathers.  K = 0 succeeds with eight zeros in d_counts and touches nothing else.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_TRACK_PLAN_COLS 8
#define ICPFLOW_TRACK_PLAN_COUNTS 4
#define ICPFLOW_REPAIR_COLS 12
#define ICPFLOW_REPAIR_COUNTS 8
typedef struct icpflow_repair_params {
    size_t struct_size;       /* sizeof(icpflow_repair_params_t) */
    double translation_frame; /* the association's bound on the translation norm, metres; default 2.0 */
    double thres_iou;         /* ... on min(iou); default 0.2 */
    double rot_limit_deg;     /* ... on the two tested angles, degrees (thres_rot * 90); default 9.0 */
    double thres_error;       /* ... on min(error), metres; default 0.2 */
    double max_residual;      /* metres: the new displacement lies this close to the predicted one in xy; default 0.2 */
} icpflow_repair_params_t;
int icpflow_object_tracks_suspects(const double *d_obs, int M, int T, const icpflow_track_params_t *params, double *d_plan,
                                   int64_t *d_counts, icpflow_stream_t stream);
int icpflow_pairs_repair_default_params(icpflow_repair_params_t *params);
int icpflow_pairs_repair_select(const float *d_T_new, const float *d_T_old, const int32_t *d_iters, const float *d_errors,
                                const float *d_ious, const float *d_translations, const float *d_rotations,
                                const float *d_errors_old, const double *d_centre, const double *d_pred, int K,
                                const icpflow_repair_params_t *params, float *d_T_out, double *d_report, int64_t *d_counts,
                                icpflow_stream_t stream);
size_t icpflow_pairs_reregister_workspace_bytes(int K, int N);
int icpflow_pairs_reregister(const icpflow_tables_t *tables, int K, int N, const int64_t *d_seg, float *d_clouds,
                             const float *d_init, const float *d_T_old, const double *d_centre, const double *d_pred,
                             const icpflow_registration_t *reg, const icpflow_repair_params_t *params, float *d_T_out,
                             double *d_report, int64_t *d_counts, void *d_ws, size_t ws_bytes, icpflow_stream_t stream,
                             const icpflow_options_t *opt);

/* ---------------------------------------------------------------------------
 * 8(n)  track fill: the gap in which a track found no pair registered from what the other gaps predict.  A cluster the
 * association missed in one gap is in no pair row, and the flow gives its points the ego motion only.  Where the same object
 * was registered in two or more other gaps that agree on one velocity, they predict where its source cluster lies in the
 * missing gap, which destination cluster it belongs to (the segment of the shared sweep that carries the track's id in that
 * gap's labelling) and the translation to start ICP from; icpflow_pairs_reregister (8(m)) registers the pair from there, with
 * T_old the identity -- the cluster unmoved, which is what the flow gave it -- and its select decides.  Multi-frame samples
 * only.  No counterpart in the reference; which (track, gap) is filled, with which source cluster, and the acceptance rule
 * are stated policies (COVERAGE.md, named deviations).
 *
 * icpflow_object_tracks_missing -- which segment of the shared sweep lacks a pair in its gap, over all gap slots at once:
 *   d_obs double [M][ICPFLOW_TRACK_OBS_COLS], M, T and params as icpflow_object_tracks_suspects takes them (only max_residual
 *   is read); d_segments double [G][Lmax][ICPFLOW_TRACK_SEGMENT_COLS] and d_num int32 [G]: what icpflow_object_tracks_extend
 *   left per gap slot, concatenated; h_gap int32 [G] and h_seconds double [G] (HOST), 1 <= G <= ICPFLOW_TRACK_MISSING_MAX_SLOTS:
 *   the gap value the observations of slot g carry in column 1, and the seconds the slot spans -- copied before the call
 *   returns (they travel in the kernel arguments).  One thread per (slot g, segment c < min(d_num[g], Lmax)); the arithmetic
 *   is the suspects' (one device function walks for both): fp64, every operation written out, no fma, rows ascending.
 *   t = column 2 of the segment; the segment HAS AN ID iff 0 <= t < T.  First walk, over the rows i whose column 0 equals t:
 *   a row with gap_i == h_gap[g] makes the segment OBSERVED -- it is counted and enters nothing else; for every other row
 *   A += s_i s_i; B += s_i d_i per axis; L += (c_i + d_i) per axis, c columns 10-12 (one addition, then the accumulation);
 *   the bit of gap_i is set for a gap in [0, 63]; others += 1.  The segment is ELIGIBLE iff it is not observed, at least two
 *   distinct gaps were seen and A > 0; then v = B / A.  Second walk, over the same rows: inner = the largest
 *   (dx_i - s_i vx)^2 + (dy_i - s_i vy)^2.  p = h_seconds[g] v; q = L / others - p (the mean landing point on the shared sweep,
 *   moved back by p: the predicted centre of the source box); m2 = max_residual * max_residual (one product).  MISSING iff
 *   eligible and inner <= m2.  Row (g, c) of d_plan double [G][Lmax][ICPFLOW_TRACK_MISSING_COLS]:
 *       0  missing    1  t    2  the segment's label    3  rows observed in this gap    4  others    5  distinct gaps
 *       6-8  p        9-11  q                           12  sqrt(inner)                  13  the segment's rows
 *   (columns 0 and 6-12 are zero for a row that is not eligible, 3-5 too for a segment without an id).  Rows from d_num[g] on
 *   are not written; a slot with a negative d_num[g] writes none.  d_counts int64 [G][ICPFLOW_TRACK_MISSING_COUNTS]: segments
 *   with an id, of them not observed, eligible, missing; by ballot and popcount, integer atomics only.  One launch, no
 *   workspace, asynchronous on `stream`.  Refusals, before any launch: a null required pointer (d_obs with M > 0, every other
 *   one), M < 0, T < 0, G outside [1, 64], Lmax < 1, h_gap values outside [0, 63] or not distinct, seconds not positive and
 *   finite, a struct_size mismatch, a negative or non-finite max_residual are ICPFLOW_E_ARG; M > 2^16, T > 2^24 or Lmax > 4096
 *   is ICPFLOW_E_LIMIT.
 *
 * icpflow_pairs_fill_candidates -- the source cluster of each missing row of ONE gap:
 *   d_q double [K][3]: columns 9-11 of the K missing rows; d_boxes_src double [Lmax][ICPFLOW_BOX_COLS] and d_num_src:
 *   icpflow_segment_boxes' table of the ego-compensated source (a count above Lmax is read as Lmax, a negative one as 0);
 *   d_pair_rows float32 [P][pair_stride], pair_stride >= 1: column 0 the source labels already matched; radius (metres) in
 *   (0, 1e3]; max_rows >= 1.  Segment c is a CANDIDATE iff its column 3 >= 0 (it has a box), its column 1 <= max_rows, and its
 *   label narrowed to float equals no column 0 of the pair rows (IEEE ==: +0 and -0 are one label, a NaN equals none; the pair
 *   rows pass through LDS in tiles of 1024).  For row k: dx = X_c - q_x, dy = Y_c - q_y (box columns 6, 7),
 *   d2 = dx dx + dy dy in fp64 without fma; the candidate is WITHIN REACH iff d2 <= radius * radius (one product; a NaN is
 *   not).  The CHOICE of row k is the reachable candidate with the smallest d2, ties to the lower c.  Where several rows
 *   choose one segment the row with the smallest d2 keeps it, ties to the lower k; the others LOSE it and get no second
 *   choice.  Row k of d_choice double [K][ICPFLOW_FILL_CHOICE_COLS]:
 *       0  reason: 0 chosen, 1 none within reach, 2 lost    1  the segment, or -1 (a loser names the segment it lost)
 *       2  its label    3  its rows    4  sqrt(d2)    5-7  its box centre (columns 6-8)        (1-7: -1 and zeros for reason 1)
 *   d_counts int64 [ICPFLOW_FILL_COUNTS]: chosen, none, lost, candidates.  Two launches: a 256-thread workgroup per row strides
 *   over the segments, the minimum of (d2, c) goes through the wave and then LDS -- a minimum does not depend on the order, so
 *   the result is a function of the arguments alone --; a thread per row then settles the shared choices.  No workspace, no
 *   floating-point atomic, asynchronous on `stream`.  Refusals, before any launch: a null required pointer (d_boxes_src,
 *   d_num_src, d_counts; d_q and d_choice with K > 0), K < 0, P < 0, Lmax < 1, pair_stride < 1, P > 0 with no pair rows, a radius
 *   outside (0, 1e3] (a NaN too), max_rows < 1 are ICPFLOW_E_ARG; K > 2^16 or Lmax > 4096 is ICPFLOW_E_LIMIT.  K = 0 succeeds
 *   with four zeros.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_TRACK_MISSING_COLS 14
#define ICPFLOW_TRACK_MISSING_COUNTS 4
#define ICPFLOW_TRACK_MISSING_MAX_SLOTS 64
#define ICPFLOW_FILL_CHOICE_COLS 8
#define ICPFLOW_FILL_COUNTS 4
int icpflow_object_tracks_missing(const double *d_obs, int M, int T, const double *d_segments, const int32_t *d_num, int G,
                                  int Lmax, const int32_t *h_gap, const double *h_seconds,
                                  const icpflow_track_params_t *params, double *d_plan, int64_t *d_counts,
                                  icpflow_stream_t stream);
int icpflow_pairs_fill_candidates(const double *d_q, int K, const double *d_boxes_src, const int32_t *d_num_src, int Lmax,
                                  const float *d_pair_rows, int P, int pair_stride, double radius, int max_rows,
                                  double *d_choice, int64_t *d_counts, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * 8(f)  ground segmentation of one cloud: the method of Patchwork++ as the reference configures it -- a fresh object for
 * every cloud (utils_ground.py:52-58), so the adaptive elevation and flatness thresholds stay {0,0,0,0} during the only
 * call; RNR off, R-VPF and TGR on.  A restatement of the method in fp64, not of Eigen's fp32 bits (COVERAGE.md, named
 * deviations).
 *
 * icpflow_ground_default_params -- replaces utils_ground.py:52-57 and the constructor defaults of patchworkpp.h:75-107.
 * icpflow_ground_segment -- replaces utils_ground.py:43-66 (segment_ground_pypatchworkpp) = estimateGround of
 *   patchworkpp.cpp:141-319 with pc2czm :561-605, extract_initial_seeds :67-139, estimate_plane :37-65,
 *   extract_piecewiseground :450-532, temporal_ground_revert :385-447 and calc_mean_stdev :540-549.
 *   d_points float32 [n] rows of `stride` >= 3 floats (x, y, z first); d_nonground uint8 [n]: 1 = non-ground (rows out of
 *   range, rows with a non-finite coordinate and the rows of patches with fewer than num_min_pts points are non-ground).
 *   d_patch_table (may be NULL) float64 [ICPFLOW_GROUND_PATCHES][ICPFLOW_GROUND_TABLE_COLS]; patch = the zone's first patch
 *   (0, 32, 160, 376) + ring * sectors + sector; columns:
 *       0      points of the patch                      1      points of its ground part (R-GPF's last round)
 *       2-4    mean of the last plane estimate           5-7    its normal (normal_z >= 0)
 *       8-10   its singular values, descending           11     d = -normal . mean
 *       12     the decision, ICPFLOW_GROUND_*            13     the revert, ICPFLOW_GROUND_TGR_*
 *       14     points R-VPF removed                      15     0
 *   A patch with fewer than num_min_pts points has its count and zeros.  A plane estimated from a single point is NaN
 *   (0 / 0, IEEE): every comparison with it is false and the patch ends non-ground.
 *   The workspace is the caller's: icpflow_ground_workspace_bytes(n, params) bytes, 8-byte aligned; nothing in it is read
 *   before it is written; fewer bytes are ICPFLOW_E_WORKSPACE before anything is written.  Asynchronous on `stream`, no host
 *   round trip.  n == 0 succeeds and writes nothing.  The result is a function of the arguments alone: fixed reduction
 *   orders, no floating-point atomics, a patch's points in row order (csrc/ground.hip).  One zone layout is built: rings
 *   {2,4,4,4}, sectors {16,32,54,32}, 4 rings of interest; any other is ICPFLOW_E_ARG ("zone layout").
 * ------------------------------------------------------------------------- */
#define ICPFLOW_GROUND_PATCHES 504
#define ICPFLOW_GROUND_TABLE_COLS 16
#define ICPFLOW_GROUND_TOO_FEW 0     /* fewer than num_min_pts points: non-ground      */
#define ICPFLOW_GROUND_NOT_UPRIGHT 1 /* normal_z <= uprightness_thr: non-ground        */
#define ICPFLOW_GROUND_FAR 2         /* upright, outside the rings of interest: ground */
#define ICPFLOW_GROUND_HEADING 3     /* mean . normal >= 0: non-ground                 */
#define ICPFLOW_GROUND_ACCEPTED 4    /* mean_z < 0 (or flat): ground                   */
#define ICPFLOW_GROUND_CANDIDATE 5   /* decided by the temporal ground revert          */
#define ICPFLOW_GROUND_TGR_NONE 0
#define ICPFLOW_GROUND_TGR_REVERTED 1 /* back to ground */
#define ICPFLOW_GROUND_TGR_REJECTED 2 /* non-ground     */
typedef struct icpflow_ground_params {
    size_t struct_size;                    /* sizeof(icpflow_ground_params_t) */
    double sensor_height;                  /* 1.723  (utils_ground.py:55) */
    double min_range;                      /* 1.0    (utils_ground.py:56) */
    double max_range;                      /* 64     (utils_ground.py:57) */
    double th_seeds;                       /* 0.125 */
    double th_dist;                        /* 0.125 */
    double th_seeds_v;                     /* 0.25 */
    double th_dist_v;                      /* 0.1 */
    double uprightness_thr;                /* 0.707 */
    double adaptive_seed_selection_margin; /* -1.2 */
    int num_iter;                          /* 3 */
    int num_lpr;                           /* 20 */
    int num_min_pts;                       /* 10 */
    int num_rings_of_interest;             /* 4 */
    int num_sectors_each_zone[4];          /* {16, 32, 54, 32} */
    int num_rings_each_zone[4];            /* {2, 4, 4, 4} */
} icpflow_ground_params_t;
int icpflow_ground_default_params(icpflow_ground_params_t *params);
size_t icpflow_ground_workspace_bytes(int n, const icpflow_ground_params_t *params);
int icpflow_ground_segment(const float *d_points, int stride, int n, const icpflow_ground_params_t *params,
                           uint8_t *d_nonground, double *d_patch_table, void *d_ws, size_t ws_bytes,
                           icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * Diagnostics: the vote kernels evaluate (v - min) / (max - min) with the loop-invariant part of
 * the IEEE division hoisted (hist.hip, AxisQuot).  For numerators d_a [n] this returns that
 * quotient (d_fast) next to the compiler's correctly rounded a / (max - min) (d_ieee); the two
 * must be bit-identical (hist_cuda_core.cuh:52-54 is an IEEE division).
 * ------------------------------------------------------------------------- */
int icpflow_selftest_vote_quotient(const float *d_a, int n, float min_v, float max_v, float *d_fast,
                                   float *d_ieee, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * Diagnostics: the Kabsch solve of the ICP iteration alone (the kernels' own code, csrc/kabsch.hpp
 * kabsch_mirror / kabsch_solve / kabsch_unmirror), one wave per matrix.  d_H [n][9]: H = sum w x_c y_c^T / W
 * (row-major, row-vector convention y = x R); d_gsum [n]: Newton's start, an upper bound of 2 (s1 + s2 + s3)
 * -- what icpflow_icp passes is (sum w |x_c|^2 + sum w |y_c|^2) / W.  mode 0: as icpflow_icp; mode 1: as
 * icpflow_icp with allow_reflection; mode 2: as the fp32-reference arithmetic, whose start is 2 sqrt(3) |H|_F
 * (d_gsum unused, may be NULL).  Out: d_R [n][9] (y = x R), d_lam [n]: Newton's root of the closed form, sum_ij R_ij H_ij
 * on the rank-1 path (icpflow_icp's scale takes sum_ij R_ij H_ij on both), d_path [n]:
 * 0 = closed form (Horn), 2 = rank-1 fallback (rotation from u to v; R = I for H = 0).
 * ------------------------------------------------------------------------- */
int icpflow_selftest_kabsch(const double *d_H, const double *d_gsum, int n, int mode, double *d_R, double *d_lam,
                            int32_t *d_path, icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * Diagnostics: the peak search as icpflow_estimate_init_pose / icpflow_hist_icp run it (hist.hip, launch_hist_peaks_u32):
 * d_bins_u32 uint32 [B, len_x, len_y, len_z], the vote's counters as they are, compared as integers (any value of uint32_t
 * but 2^32 - 1 in bin 0 of a volume: that bin's selection key, all ones, is the selection's "nothing taken yet"; a vote
 * counts pairs of points and stays far below); k, kernel_size, d_votes, d_idx, d_ws / ws_bytes and the order as
 * icpflow_hist_peaks (d_votes is float32 of the integer vote).
 * d_cand: NULL, or float32 [B, k + 1, 3]: candidate r of pair b is (d_edges_x[ix] + decode_shift, d_edges_y[iy] +
 * decode_shift, d_edges_z[iz] + decode_shift) of peak r's bin (ix, iy, iz), each one float32 addition; the zero
 * translation comes last.  d_edges_* float32 [len_*] are read only with d_cand.
 * ------------------------------------------------------------------------- */
int icpflow_selftest_peaks_u32(const uint32_t *d_bins_u32, int B, int len_x, int len_y, int len_z, int k, int kernel_size,
                               const float *d_edges_x, const float *d_edges_y, const float *d_edges_z, float decode_shift,
                               float *d_votes, int64_t *d_idx, float *d_cand, void *d_ws, size_t ws_bytes,
                               icpflow_stream_t stream);

/* ---------------------------------------------------------------------------
 * Diagnostics, host only (no launch, no device access): byte offsets, from the d_ws a fused entry point
 * (icpflow_estimate_init_pose, icpflow_hist_icp, icpflow_icp, icpflow_apply_icp; the same B, N and histogram
 * lengths, 0 0 0 for the two without a histogram) was given, of the arrays its sorts leave there.  Once the call
 * has returned and the stream is synchronised the arrays are still in the caller's workspace.  h_offsets [count],
 * count = ICPFLOW_WORKSPACE_LAYOUT_COUNT (anything else is ICPFLOW_E_ARG), in this order:
 *    0 lenA      int32 [B]   valid rows of the src cloud          1 lenC   int32 [B]   ... of the dst cloud
 *    2 swap      uint8 [B]   1: the src cloud is the longer one and takes the fixed role (icpflow_hist_icp only)
 *    3 grid.pts  float [B,N,4]  the fixed role's cloud sorted along the pair's key: (x, y, z, row as int bits)
 *    4 grid.sortX float [B,N,4] the moving role's cloud (pre-pose applied), the same key and layout
 *    5 grid.sortYsoa float [B,3,NP16]  x[], y[], z[] of 3, +inf behind the valid rows; NP16 = N rounded up to 16
 *    6 grid.sortXsoa float [B,3,NP16]  the same of 4 (where the call sorts for the scoring sweeps)
 *    7 grid.axis int32 [B]   the pair's key code: 0 1 2 = x y z, 3 .. 8 = a horizontal direction (csrc/sortdir.hpp)
 *    8 zsortA    float [B,N,4]  the src cloud's flagged rows by the vote's key, the key in w
 *    9 zsortC    float [B,N,4]  ... the dst cloud's             10 voteKey float [B,8]  wide, uaxis, u0, z0, h (csrc/votekey.hpp)
 * icpflow_hist_icp_eval reuses zsortA behind the registration.
 * ------------------------------------------------------------------------- */
#define ICPFLOW_WORKSPACE_LAYOUT_COUNT 11
int icpflow_selftest_workspace_layout(int B, int N, int Lx, int Ly, int Lz, size_t *h_offsets, int count);

/* ---------------------------------------------------------------------------
 * Measurement aid (no reference counterpart): per-launch timing of the dominant kernel, the ICP
 * iteration.  A recorder is an object the caller owns: every launch of that kernel made by a call
 * that carries it in its options (up to `capacity` launches) is bracketed by HIP events recorded on
 * the caller's stream; icpflow_profile_collect() waits for the recorded events, returns the summed
 * duration in milliseconds and the number of launches, and re-arms the recorder.  One recorder must
 * not be used by two host threads at once; distinct recorders are independent.
 * ------------------------------------------------------------------------- */
int icpflow_profile_create(int capacity, icpflow_profile_t **out);
int icpflow_profile_collect(icpflow_profile_t *profile, double *total_ms, int *launches);
int icpflow_profile_destroy(icpflow_profile_t *profile);

#ifdef __cplusplus
}
#endif
#endif /* ICPFLOW_HIP_H */
