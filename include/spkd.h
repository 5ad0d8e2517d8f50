/*
 * spkd.h — C ABI of libspkd_hip.so: BIC / GLR / KL2 speaker-change detection and
 * agglomerative clustering on Gaussian sufficient statistics, hand-written HIP
 * for gfx950 (MI355X).
 *
 * The reference (JianCao92/speaker-diarization) has no FFI: its hot path is
 * Python calling numpy.cov / scipy.linalg.det per distance.  Each entry point
 * below names the reference function(s) whose arithmetic it replaces, so a
 * maintainer can bind it with ctypes from the scripts of the same name (see
 * INTEGRATION.md).  Conventions:
 *   - plain C, caller-owned buffers, no global state, one context per
 *     (device, stream); a context is not re-entrant, different contexts are
 *     independent;
 *   - pointer arguments are prefixed d_ (device memory) or h_ (host memory);
 *   - every call returns an spkd_status; spkd_last_error() gives the text;
 *   - every call returns with the work it enqueued finished, whatever its status;
 *   - all scores are IEEE binary64; frames are binary32 exactly as feacat wrote
 *     them (spk-change-detection.py:37-41).
 *
 * Statistics record ("stats"): SPKD_REC = 820 doubles, the packed upper triangle
 * (row-major, r <= c) of the augmented second-moment matrix sum([x;1][x;1]^T)
 * of a frame set, d = 39: entry (r, c) at r*40 - r*(r-1)/2 + (c - r);
 * (r, 39) = sum x_r, (39, 39) = frame count.  Records add component-wise under
 * set union, which is what replaces the reference's np.concatenate + np.cov.
 */
#ifndef SPKD_H
#define SPKD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPKD_ABI_VERSION 2
#define SPKD_DIM 39
#define SPKD_REC 820

typedef enum {
    SPKD_OK = 0,
    SPKD_EINVAL = 1,      /* bad argument / unsupported parameter combination */
    SPKD_EHIP = 2,        /* a HIP runtime call failed */
    SPKD_ENONFINITE = 3,  /* a covariance was NaN/inf: the reference raises ValueError there */
    SPKD_EOVERFLOW = 4,   /* an output / log buffer was too small; *needed is set */
    SPKD_ENOMEM = 5
} spkd_status;

typedef enum { SPKD_BIC = 0, SPKD_GLR = 1, SPKD_KL2 = 2, SPKD_KL2_PINV = 3 } spkd_kind;

/* KL2 modes.  The reference's kl2 (spk-clustering.py:124-133, spk-change-detection.py:124-133)
 * uses only diag(scipy.linalg.pinv(S)) of each covariance.
 *   SPKD_KL2 (the default): diag(S^-1) by an elimination without pivoting; NaN whenever S is
 *     not positive definite (digital silence, constant stretches, any set of fewer than 40
 *     frames), so such a distance is NaN where the reference's is finite.
 *   SPKD_KL2_PINV (opt-in): the reference's pseudo-inverse.  Eigenvalues with
 *     |lambda| > 39 * eps * max|lambda| are kept (strictly greater: an all-zero covariance
 *     has a zero pseudo-inverse, as in scipy), diag_i = sum over kept k of V_ik^2 / lambda_k.
 *     Positive definite covariances with tr(S) tr(S^-1) <= 1e-3 / (39 eps) keep every
 *     eigenvalue and take the inverse's diagonal as in SPKD_KL2; the others go through a
 *     one-wave Jacobi eigen-decomposition on the device, which gives NaN if it has not
 *     converged after 40 sweeps.  Non-finite covariances behave as in SPKD_KL2 and return
 *     SPKD_ENONFINITE where that does (scipy's pinv refuses them too).  The covariance is
 *     formed from the sufficient statistics: a constant stretch whose frames are not all
 *     zero gives a covariance of rounding noise instead of an exact zero, and the distance
 *     then differs from the reference's (BIC's log det has the same limit).
 *   The first call in this mode allocates the context's Jacobi workspace (about 26 MB of
 *   device memory, freed by spkd_destroy). */

typedef struct spkd_ctx spkd_ctx;

int spkd_abi_version(void);

/* device = HIP device ordinal; stream = a hipStream_t to launch on, or NULL for a
 * stream owned by the context.  The owned stream is a blocking one: it is ordered
 * with work on the legacy default stream (handle 0, which is also what torch's
 * default stream is), not with other non-blocking streams.
 * spkd_create_on_stream always launches on the given handle, NULL included (NULL =
 * the legacy default stream): this is the call for "the caller's current torch
 * stream", whose handle is 0 unless the caller made a stream of its own. */
spkd_status spkd_create(int device, void *stream, spkd_ctx **out);
spkd_status spkd_create_on_stream(int device, void *stream, spkd_ctx **out);
void spkd_destroy(spkd_ctx *ctx);
const char *spkd_last_error(const spkd_ctx *ctx);
spkd_status spkd_sync(spkd_ctx *ctx);

/* Device memory helpers so a ctypes-only host can run without torch. */
spkd_status spkd_malloc(spkd_ctx *ctx, size_t bytes, void **d_ptr);
spkd_status spkd_free(spkd_ctx *ctx, void *d_ptr);
spkd_status spkd_memcpy_h2d(spkd_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
spkd_status spkd_memcpy_d2h(spkd_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
spkd_status spkd_memcpy_d2d(spkd_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);

/* Timing of the most recent call, measured with HIP events recorded on the
 * context's stream around each kernel launch (milliseconds).
 * which: SPKD_T_CALL = whole call; SPKD_T_<kernel> = that kernel's launch inside
 * the most recent call that used it. */
enum {
    SPKD_T_CALL = 0, SPKD_T_CHUNK_STATS, SPKD_T_REDUCE_SETS, SPKD_T_PAIR_TERMS,
    SPKD_T_CLUSTER_PREP, SPKD_T_MATRIX, SPKD_T_AHC, SPKD_T_GW, SPKD_T_SW, SPKD_T_MERGE,
    SPKD_T_VAD_SHIFT, SPKD_T_VAD_VITERBI, SPKD_T_VAD_BACKTRACK, SPKD_T_GAUSS_MODELS, SPKD_T_GAUSS_LOGLIK,
    SPKD_T_POST_STATS, SPKD_T_BF_GCC, SPKD_T_BF_TRACK, SPKD_T_BF_SUM, SPKD_T_RESAMPLE, SPKD_T_FRAME_ENERGY, SPKD_T_ENERGY_SEEDS,
    SPKD_T_FEATURE_WARP, SPKD_T_TDOA_PACK, SPKD_T_TDOA_STATS, SPKD_T_TDOA_MODELS, SPKD_T_TDOA_SCORE,
    SPKD_T_TDOA_CUTS, SPKD_T_TDOA_SPLIT, SPKD_T_TDOA_SECOND, SPKD_T_TDOA_OVERLAP,
    SPKD_T_GMM_TRAIN, SPKD_T_GMM_SEQ_LOGLIK, SPKD_T_UBM_STATS, SPKD_T_CLR_LINK,
    SPKD_T_MINDUR_VITERBI, SPKD_T_MINDUR_BACKTRACK, SPKD_T_FB_POSTERIOR,
    SPKD_T_IDENT_SCORES, SPKD_T_IDENT_ASSIGN, SPKD_T_BW_ACCUMULATE,
    SPKD_T_MFCC_STATIC, SPKD_T_MFCC_POST,
    SPKD_N_TIMERS
};
spkd_status spkd_last_kernel_ms(spkd_ctx *ctx, int which, float *ms);

/* Work done by the most recent growing-window call (spkd_gw / spkd_gw_ex / spkd_gw_fused):
 * the number of 39x39 determinants it evaluated (one per covariance the reference's bic /
 * glr form at spk-change-detection.py:87-98, 107-115 -- left, right, pooled, within).
 * For the fp64 figure beside the HBM fraction. */
spkd_status spkd_last_gw_items(spkd_ctx *ctx, int64_t *items);

/* ---------------------------------------------------------------------------
 * (1) Sufficient statistics of frame sets.
 * Replaces get_spk_features + np.cov inputs (spk-clustering.py:46-52,88-94).
 * A set is the concatenation of one or more frame ranges [begin, end); ranges
 * of one set are contiguous in the arrays and set ids are non-decreasing.
 * d_stats receives n_sets records of SPKD_REC doubles.
 *
 * Accuracy domain.  A record holds RAW moments (n, sum x_i, sum x_i x_j); each entry is within
 * (n + 64) 2^-53 sum_t |x_ti x_tj| of the exact sum (asserted against exact integer arithmetic,
 * tests/test_conditioned_exact.py).  Every covariance downstream is (M - s s^T / n) / (n - 1),
 * which cancels about 2 log10(mean / sigma) digits that np.cov, subtracting the mean first, keeps.
 * With means within a few sigma of zero this is as accurate as the reference; a caller whose
 * features are not centred subtracts one constant vector per file from every frame first
 * (covariances do not change under a shift).  DESIGN.md section 4, "Accuracy domain".
 */
spkd_status spkd_set_stats(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                           const int64_t *h_range_begin, const int64_t *h_range_end,
                           const int32_t *h_range_set, int64_t n_ranges,
                           int64_t n_sets, double *d_stats);

/* ---------------------------------------------------------------------------
 * (2) Distance terms of set pairs.
 * Replaces the bodies of bic / glr / kl2 (spk-clustering.py:81-133,
 * spk-change-detection.py:72-133) for callers that keep the decision on the
 * host (merge_rec, spk_cluster_in).  For pair p the 8 doubles at h_terms[8*p]:
 *   [0] n1  [1] n2  [2] log det S1  [3] log det S2  [4] log det S(union)
 *   [5] log det((n1 S1 + n2 S2)/N)   (only with SPKD_WANT_GLR, else NaN)
 *   [6] KL2 as coded in the reference (only with SPKD_WANT_KL2 or SPKD_WANT_KL2_PINV, else NaN)
 *   [7] reserved
 * S = np.cov(rowvar=0) semantics (unbiased); log det = log of the LU
 * determinant: 0 -> -inf, negative -> NaN.
 *
 * Accuracy domain (against exact arithmetic on full-rank sets of 40 to 3 000 frames; measure
 * |a - b| / max(1, |a|, |b|) over the log-dets and the BIC / GLR assembled from them; table in
 * DESIGN.md section 4): covariances of cond <= 5e2 with means up to 8 sigma: 1e-9; means of 64 sigma,
 * or cond 1e6 with means up to 64 sigma, or cond 1e9 with means up to 8 sigma: 1e-5 (at 8 sigma
 * with little to spare: up to 2e-6 here, 7e-6 through spkd_gw's running sums); cond 1e9 with means
 * of 64 sigma: outside 1e-5 (up to 8e-4, where the reference keeps 4e-8).  The limit is that of the raw-moment records (spkd_set_stats above), not of the
 * elimination: the kernels stay within a small multiple of the same formulation in plain C.
 */
#define SPKD_WANT_GLR 1
#define SPKD_WANT_KL2 2
#define SPKD_WANT_KL2_PINV 4   /* term [6] is SPKD_KL2_PINV's KL2; excludes SPKD_WANT_KL2 (SPKD_EINVAL) */
spkd_status spkd_pair_terms(spkd_ctx *ctx, const double *d_stats,
                            const int32_t *h_idx_a, const int32_t *h_idx_b,
                            int64_t n_pairs, int flags, double *h_terms);

/* Full symmetric n x n distance matrix of one kind from n records
 * (the initial double loop of spk_cluster_hi, spk-clustering.py:188-200);
 * diagonal = 2^63 (sys.maxint as a float).  d_matrix: n*n doubles. */
spkd_status spkd_distance_matrix(spkd_ctx *ctx, int kind, double lambdac,
                                 const double *d_stats, int64_t n, double *d_matrix);

/* spk_cluster_in (spk-clustering.py:136-175, spk-clustering2.py:135-170) over n statistics
 * records in recipe order, as one device-resident chain: record 0 founds cluster 0; every
 * later record is compared with every cluster so far (the cluster is the distance's first
 * argument, the record its second; a cluster's record is the sum of its members') and joins
 * the first arg-min over the finite distances if that is <= threshold, else founds a cluster.
 * kind: SPKD_BIC, SPKD_GLR, SPKD_KL2 or SPKD_KL2_PINV.  h_label[n]: 0-based cluster of every record.  h_dist
 * [dist_cap]: all distances in evaluation order, those of record s at h_dist_off[s] ..
 * h_dist_off[s + 1] (h_dist_off[n + 1]) -- the caller replays the reference's prints and
 * statistics from them.  *h_n_done: records processed; < n with SPKD_ENONFINITE (a
 * covariance with infs or NaNs at record *h_n_done: the reference raises there, after the
 * lines before it were written) or SPKD_EOVERFLOW (dist_cap too small: call again with more;
 * n (n - 1) / 2 always fits).  *h_n_clusters: clusters founded. */
spkd_status spkd_cluster_in(spkd_ctx *ctx, const double *d_stats, int64_t n, int kind,
                            double lambdac, double threshold, int32_t *h_label,
                            double *h_dist, int64_t dist_cap, int64_t *h_dist_off,
                            int64_t *h_n_done, int64_t *h_n_clusters);

/* spkd_cluster_in for n_problems independent recipes (files) in one launch, a workgroup per
 * problem: problem p owns the records [h_seg_off[p], h_seg_off[p+1]) of d_stats (read only;
 * h_seg_off[0] = 0, n = h_seg_off[n_problems]) and is clustered exactly as spkd_cluster_in
 * clusters those records alone -- same kernels' arithmetic in the same order, the same labels
 * and distances to the bit.  The distances themselves are not returned:
 *   h_label[n]        0-based cluster of every record within its problem
 *   h_mind[n]         the reference's `mind` of the record: the minimum over its finite
 *                     distances, the value compared with the threshold; 2^63 (sys.maxint)
 *                     when it has none, as for the first record of a problem
 *   h_n_done[p], h_n_clusters[p]   records processed and clusters founded
 *   h_stat_max[p], h_stat_min[p]   max / min over every finite distance of the records
 *                     processed (NaN: none) -- the summary the scripts print
 * An empty problem reports 0 records, 0 clusters, NaN; n_problems = 0 is SPKD_OK.  A covariance
 * with infs or NaNs stops ITS problem at record h_n_done[p] < its size, like spkd_cluster_in,
 * and leaves every other problem untouched: the call returns SPKD_ENONFINITE with all outputs
 * valid (h_label -1 and h_mind NaN from the record that stopped a problem on).  There is no
 * distance buffer and so no SPKD_EOVERFLOW.  A bad kind, a null pointer, an h_seg_off that
 * decreases or a problem of more than 65 536 records: SPKD_EINVAL before any device work. */
spkd_status spkd_cluster_in_batch(spkd_ctx *ctx, const double *d_stats, int64_t n_problems,
                                  const int64_t *h_seg_off, int kind, double lambdac,
                                  double threshold, int32_t *h_label, double *h_mind,
                                  int64_t *h_n_done, int64_t *h_n_clusters,
                                  double *h_stat_max, double *h_stat_min);

/* Rows [row_begin, row_end) of that matrix, as spk_cluster_hi's variant `variant` fills them
 * (a block of the outer loop of spk-clustering.py:188-200 / spk-clustering2.py:178-184):
 * d_rows[(a - row_begin) * n + c] for c > a is the distance, c == a the diagonal value
 * (variant 1: 2^63, variant 2: +inf), c < a: +inf for variant 2, UNSPECIFIED for variant 1
 * (the caller mirrors the upper triangle).  One long file tiled over several GPUs
 * (SURVEY.md 8(e) row 2): every rank holds all n records, computes its block of rows, the
 * blocks are gathered, spkd_ahc_matrix runs the merge loop on the assembled matrix.
 * h_stat_max / h_stat_min (may be NULL): max / min over the finite distances of the block
 * (NaN: none) -- variant 1's running statistics start from the max / min over all blocks. */
spkd_status spkd_distance_rows(spkd_ctx *ctx, int variant, int kind, double lambdac,
                               const double *d_stats, int64_t n, int64_t row_begin, int64_t row_end,
                               double *d_rows, double *h_stat_max, double *h_stat_min);

/* ---------------------------------------------------------------------------
 * (3) Change detection.
 */
typedef struct {
    int32_t kind;        /* spkd_kind */
    int32_t trace;       /* 1: log every coarse candidate (-tt); 0: only infinite ones */
    double lambdac;      /* BIC penalty weight (-l) */
    double threshold;    /* -t */
    double winsize;      /* floor(w * rate), frames */
    double winstep;      /* floor(st * rate), frames */
    double deltaws;      /* floor(rate * dws), frames */
    double rate;         /* frames per second (-f) */
} spkd_cd_params;

typedef struct {         /* one logged candidate evaluation */
    int32_t turn;
    int32_t coarse;      /* 1 = coarse scan, 0 = fine-tune scan */
    int64_t seq;         /* (scan index << 32) | candidate index; bit 31 set = fine-tune scan */
    double start, i, d;
    int64_t n1, n2;
} spkd_cand_log;

/* Growing-window detector, dist_gw (spk-change-detection.py:180-288), all turns
 * of one feature array in one launch, one workgroup (few turns) or one wave (thousands of
 * turns) per turn -- the results are bit-identical.
 * Per turn t the events land at [h_ev_off[t], h_ev_off[t+1]) of the h_win_ and
 * h_det_ arrays; spkd_gw checks capacity per turn >= spkd_gw_event_capacity_p(len, params)
 * (a first guess, see below: SPKD_EOVERFLOW asks for more).
 * winstep < 1 frame is rejected (the reference's loop does not terminate there).
 *   h_n_win[t]           number of coarse scans (outer iterations)
 *   h_win_maxd[...]      best coarse distance of each scan (NaN: none accepted)
 *   h_win_det[...]       1 if that scan ended in a detection
 *   h_det_start/maxi/d   one triple per detection, in order
 *   h_final_start[t]     `start` when the loop ended (the tail line starts here)
 * h_log may be NULL (log_cap 0); *h_log_count receives the number of records the
 * run wanted to write (SPKD_EOVERFLOW if > log_cap).
 * Device scratch held by the context: one SPKD_REC record (6 560 bytes) of running
 * moment sums per candidate slot, about turn_len / (rate / 10) slots per turn (0.52 KB
 * per frame).
 */
/* Event capacity per turn: a FIRST GUESS, not a bound.  Both count the scans of a window
 * end that only moves forward (turn_len / step + 8; spkd_gw_event_capacity assumes winstep >=
 * 0.2 * rate, i.e. -st >= 0.2 s, spkd_gw_event_capacity_p covers every winstep: below that
 * the window grows by winstep frames per negative scan).  After every detection the
 * reference resets the window end to start + 2 * winsize (spk-change-detection.py:264-266)
 * and the window regrows over frames already scanned, so a change point found early in a
 * long-grown window can make a turn need MORE scans.  Such a call returns SPKD_EOVERFLOW
 * (nothing is written out of bounds, no result is valid); the caller repeats it with larger
 * capacities -- any capacity >= the guess is accepted (the Python host doubles until it
 * fits).  -1 for parameters spkd_gw rejects. */
int64_t spkd_gw_event_capacity(int64_t turn_len, double rate);
int64_t spkd_gw_event_capacity_p(int64_t turn_len, const spkd_cd_params *params);
spkd_status spkd_gw(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                    const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                    const spkd_cd_params *params, const int64_t *h_ev_off,
                    int32_t *h_n_win, double *h_win_maxd, int32_t *h_win_det,
                    double *h_det_start, double *h_det_maxi, double *h_det_d,
                    double *h_final_start,
                    spkd_cand_log *h_log, int64_t log_cap, int64_t *h_log_count);

/* Same as spkd_gw; with check_capacity = 0 the per-turn capacity implied by
 * h_ev_off may also be smaller than spkd_gw_event_capacity_p() -- a turn that needs more
 * makes the call return SPKD_EOVERFLOW (nothing is written out of bounds) and the
 * caller repeats it with more. */
spkd_status spkd_gw_ex(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                       const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                       const spkd_cd_params *params, const int64_t *h_ev_off, int check_capacity,
                       int32_t *h_n_win, double *h_win_maxd, int32_t *h_win_det,
                       double *h_det_start, double *h_det_maxi, double *h_det_d,
                       double *h_final_start,
                       spkd_cand_log *h_log, int64_t log_cap, int64_t *h_log_count);

/* Fused mode: spkd_gw_ex that also leaves the packed statistics
 * record of every segment it emits, so that the clustering stage does not have to read
 * the frames again.  Turn t with n_det detections writes n_det + 1 records (the tail
 * segment [final_start, turn end) last) at d_seg_stats[(h_ev_off[t] + j) * SPKD_REC];
 * d_seg_stats must hold h_ev_off[n_turns] records (only the written ones are touched),
 * and a turn needs capacity >= n_det + 1 (else SPKD_EOVERFLOW).  Record j of a turn is
 * the moment sum of the turn frames [int(det_start[j]), int(det_start[j] + det_maxi[j]))
 * -- the caller decides per segment whether that is the range its clustering stage would
 * cut (it is, unless the 12-digit time round trip of SURVEY.md A-2 moved an edge). */
spkd_status spkd_gw_fused(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                          const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                          const spkd_cd_params *params, const int64_t *h_ev_off, int check_capacity,
                          int32_t *h_n_win, double *h_win_maxd, int32_t *h_win_det,
                          double *h_det_start, double *h_det_maxi, double *h_det_d,
                          double *h_final_start, double *d_seg_stats,
                          spkd_cand_log *h_log, int64_t log_cap, int64_t *h_log_count);

/* d_dst[h_dst_index[i]] = d_src[h_src_index[i]] for i < n, whole records
 * (h_dst_index = NULL: destination i).  Compacts the sparse output of spkd_gw_fused
 * into the contiguous per-problem layout spkd_ahc reads. */
spkd_status spkd_gather_stats(spkd_ctx *ctx, const double *d_src, int64_t n_src,
                              const int64_t *h_src_index, const int64_t *h_dst_index,
                              int64_t n, int64_t n_dst, double *d_dst);

/* Sums of whole records: set s owns the members h_member[h_set_off[s] .. h_set_off[s+1]), each
 * the index of a record of d_src (n_src records), and d_dst[s] is their entry-wise fp64 sum IN
 * MEMBER ORDER: the first member copied, every later one added to it, one chain of additions
 * per entry -- no atomics, no tree, no reordering, so the result is bit-reproducible and equals
 * a host loop that adds the same records in the same order (a set of one member is a copy).
 * A record is a raw moment sum, so this is the record of the union of the members' frame sets
 * without reading a frame: the speakers of a batch from its segments' records (the order of a
 * set's members is the caller's, and a record may be a member of several sets).
 * d_dst holds n_sets records and must not overlap d_src; both are 16-byte aligned.  The two
 * index arrays go up in one copy through pinned memory the context owns.  n_sets = 0 is SPKD_OK
 * without a launch.  A null pointer, h_set_off[0] != 0, an h_set_off that decreases, an empty
 * set, a member outside [0, n_src), overlapping or misaligned buffers: SPKD_EINVAL before any
 * device work, d_dst untouched.
 * Timer: SPKD_T_REDUCE_SETS (the kernel; like k_reduce_sets it sums records into sets). */
spkd_status spkd_sum_stats(spkd_ctx *ctx, const double *d_src, int64_t n_src,
                           const int64_t *h_member, const int64_t *h_set_off,
                           int64_t n_sets, double *d_dst);

/* The batch hand-off: spkd_gw_fused whose results stay on the device and come back as the
 * recipe lines the change-detection script writes (spk-change-detection.py:254 a detection,
 * :288 the tail), instead of as event slots for the host to walk.  Behind k_gw, in the same
 * call bracket and only when the device error word is clean, three small kernels count every
 * turn's detections from its window flags, scan them in the CALLER's turn order and write per
 * line what spkd_gw_lines with frame outputs writes -- same fields, same fp64 operations in
 * the same order: the two times, the turn, the record index h_ev_off[t] + j and the frame
 * range that record covers.  Only these compact arrays (and n_win per turn) are copied, into
 * pinned memory the context owns and reuses.  Then, on the host and in one pass over them:
 * the 12-digit round trip of the times (spkd_py2_roundtrip) and, per line, the frame range the
 * clustering script would cut from the round-tripped times (spk-clustering.py:263-292 parses
 * the line, :46-52 slices the frames: begin = min(int(t0 * rate), file_len), end = max(begin,
 * min(int(t1 * rate), file_len)), plus file_off) compared with the range the record covers;
 * the lines where they differ -- the round trip moved a boundary across a frame edge -- come
 * back as the redo list.
 *   h_turn_start_s / h_turn_end_s   the turn's times as the VAD recipe states them
 *   h_turn_file_off / h_turn_file_len   first frame and frame count of the turn's file
 *   want_index   also copy the line -> record map to the host (view.index; else NULL)
 * Every pointer of the view belongs to the context and is valid until its next spkd_gw_batch
 * (d_index: until the next spkd_gw_batch or spkd_ahc_fused, which consumes it).  Capacities,
 * SPKD_EOVERFLOW and d_seg_stats as for spkd_gw_fused with check_capacity = 0; no candidate
 * log.  The view is zeroed on every status but SPKD_OK. */
typedef struct {
    int64_t n_lines;             /* sum over turns of detections + 1 */
    int64_t n_redo;
    const int32_t *n_win;        /* [n_turns] */
    const double *times;         /* [n_lines][2] start, end in seconds, after the round trip */
    const int32_t *turn;         /* [n_lines] */
    const int64_t *frame_b;      /* [n_lines] range of the frame array the fused record covers */
    const int64_t *frame_e;
    const int64_t *index;        /* [n_lines] record of the line in d_seg_stats (want_index) */
    const int64_t *d_index;      /* the same map, DEVICE memory */
    const int64_t *redo_line;    /* [n_redo] ascending */
    const int64_t *redo_begin;   /* [n_redo] the range to compute the record from instead */
    const int64_t *redo_end;
} spkd_gw_lines_view;

spkd_status spkd_gw_batch(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                          const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                          const spkd_cd_params *params, const int64_t *h_ev_off,
                          const double *h_turn_start_s, const double *h_turn_end_s,
                          const int64_t *h_turn_file_off, const int64_t *h_turn_file_len,
                          double *d_seg_stats, int want_index, spkd_gw_lines_view *view);

/* Sliding-window distances, the per-window part of dist_sw
 * (spk-change-detection.py:304-312): window w of turn t compares
 * [int(w*step), int(w*step+size)) with [int(w*step+size), int(w*step+2*size)).
 * h_d receives the distances of turn t at [h_d_off[t], h_d_off[t+1]);
 * the count per turn is spkd_sw_window_count(len, size, step).
 * kind = SPKD_BIC evaluates a correct two-window BIC (the reference's own
 * sliding-window BIC path crashes). */
int64_t spkd_sw_window_count(int64_t turn_len, double winsize, double winstep);
spkd_status spkd_sw(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                    const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                    const spkd_cd_params *params, const int64_t *h_d_off, double *h_d);

/* The positive-run pass of dist_sw (spk-change-detection.py:299-357) on the device, over a
 * DEVICE array of window distances: turn t owns d_dist[h_d_off[t] .. h_d_off[t+1]) (h_d_off[0]
 * = 0), one wave per turn.  The state machine is the script's, in fp64: bestd = -1 and
 * best_position = -1 at first; d < threshold or d = +-inf is a negative window, everything else
 * (NaN included) a positive one; a positive d moves last_positive, only d > bestd moves bestd
 * and best_position = start + winsize; a series is written when start - winstep ==
 * last_positive, at a negative window and once behind the loop; writing resets bestd to 0 and
 * leaves best_position (a series that never beat bestd writes the stale position, -1 when
 * there never was one).  Uses params->winsize, winstep, threshold.
 * Results in the growing-window event layout, so that spkd_gw_lines writes the script's lines:
 * detection j of turn t at slot h_ev_off[t] + j with det_start = `end` before it, det_maxi =
 * best_position - end, det_d = bestd; h_final_start[t] = the last `end`; h_n_det[t].  A turn
 * needs (windows / 2 + 1) slots -- a bound: two series have a negative window between them --
 * and less is SPKD_EINVAL.
 * Per turn also the script's summary counters over that turn alone, each started where the
 * script starts it (maxima at 0, minima at 2^63 = float(sys.maxint)) and moved by its
 * comparisons (d > max, d < min): h_win_cnt / h_win_max / h_win_min over the windows whose
 * distance is not +-inf, h_det_max / h_det_min over the detections' det_d (their count is
 * h_n_det).  The sums are the host's: their order is. */
spkd_status spkd_sw_runs(spkd_ctx *ctx, const double *d_dist, const int64_t *h_d_off, int64_t n_turns,
                         const spkd_cd_params *params, const int64_t *h_ev_off,
                         int32_t *h_n_det, double *h_det_start, double *h_det_maxi, double *h_det_d,
                         double *h_final_start, int64_t *h_win_cnt, double *h_win_max,
                         double *h_win_min, double *h_det_max, double *h_det_min);

/* Sliding-window change detection for every turn of every file in one call: the distances of
 * spkd_sw (bit for bit: the same sums in the same order through the same kernels) and the pass
 * of spkd_sw_runs behind them, all on the device.  Only the per-turn arrays go up; the windows'
 * geometry is formed on the device.  The windows, counted flat over the turns, are processed in
 * tiles of tile_windows (0: the library's default, 4 096): device scratch is 45.8 KB per window
 * of a TILE, plus 8 bytes per window of the call for the distances -- not the 2 x 6 560 bytes
 * and the working copies per window of the call that spkd_sw needs.
 * h_d_off as for spkd_sw (checked against spkd_sw_window_count), h_ev_off and the outputs as
 * for spkd_sw_runs; only these per-turn and per-detection arrays are copied back, and the
 * distances when h_d is not NULL.  Argument checks (SPKD_EINVAL) come before any device work.
 * Frames with infs or NaNs inside a window: SPKD_ENONFINITE for the call, as spkd_sw.
 * kind = SPKD_BIC is the correct two-window BIC, as spkd_sw. */
spkd_status spkd_sw_batch(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                          const int64_t *h_turn_begin, const int64_t *h_turn_end, int64_t n_turns,
                          const spkd_cd_params *params, const int64_t *h_d_off, const int64_t *h_ev_off,
                          int64_t tile_windows,
                          int32_t *h_n_det, double *h_det_start, double *h_det_maxi, double *h_det_d,
                          double *h_final_start, int64_t *h_win_cnt, double *h_win_max,
                          double *h_win_min, double *h_det_max, double *h_det_min, double *h_d);

/* Neighbour merge, merge_rec (spk-change-detection.py:136-177, driven by :375-394: `-m m`), for
 * n_problems independent recipes (files) in one call, a device chain per problem.  Problem p owns
 * the lines [h_line_off[p], h_line_off[p+1]) of the per-line arrays (h_line_off[0] = 0, n =
 * h_line_off[n_problems]); line k covers the absolute frame range [h_line_begin[k],
 * h_line_end[k]) of d_frames.  Each problem behaves as a run of the script on that recipe alone:
 * `prev`, the run merged so far, is compared with the next line; its frames are
 * features[start_first*rate : end_last*rate], so a run spans the gaps inside it, while the gap in
 * front of the next line is not in the pooled array.  The records of all lines and all non-empty
 * gaps come from one statistics pass (each frame read once); a run is the sum of its lines' and
 * gaps' records.  That sum is only the spanning range when the lines of a problem neither overlap
 * nor go backwards (begin[k+1] >= end[k]): other recipes are SPKD_EINVAL, and the caller takes the
 * script's path for them (ChangeDetectionRun).
 * Distances in fp64 in the script's order (bic with the frozen c1 of a problem's first step,
 * SURVEY.md A-8; glr; kl2); a line joins the run before it when d < threshold and d is not +-inf.
 *   h_merged[n]   1: the line joined the run before it; 0: it starts a run (a problem's first line: 0)
 *   h_dist[n]     the distance of the step that decided the line (a problem's first line: NaN)
 *   h_n_done[p]   lines decided; less than the problem's size: the chain stopped there
 *   h_win_cnt / h_win_max / h_win_min [p]   the script's window counters over the problem's steps
 *                 whose distance is not +-inf, h_det_cnt / h_det_max / h_det_min [p] over its
 *                 merges -- started and moved as in spkd_sw_runs (maxima at 0, minima at 2^63)
 * A step whose left side or line has no finite covariance (infs or NaNs in its frames, fewer than
 * two frames) stops ITS problem at that step, as the reference's det raises there: the call
 * returns SPKD_ENONFINITE with all outputs valid (h_merged -1 and h_dist NaN from that line on)
 * and every other problem untouched.
 * The terms of every step whose left side is a line as the recipe names it are computed ahead, in
 * parallel; only the steps behind a merge are computed by the chain.  flags:
 * SPKD_MERGE_NO_AHEAD skips the ahead pass (every step computes its own terms; the results are
 * the same to the bit).  An empty problem reports 0 lines, a problem of one line that line as a
 * run without a distance; n_problems = 0 is SPKD_OK.  A null pointer, a bad kind, an h_line_off
 * that decreases, a range outside [0, n_frames] or with end < begin, overlapping lines, a problem
 * of more than 65 536 lines: SPKD_EINVAL before any device work, outputs untouched. */
#define SPKD_MERGE_NO_AHEAD 1
spkd_status spkd_merge_batch(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                             int64_t n_problems, const int64_t *h_line_off,
                             const int64_t *h_line_begin, const int64_t *h_line_end,
                             int kind, double lambdac, double threshold, int flags,
                             int32_t *h_merged, double *h_dist, int64_t *h_n_done,
                             int64_t *h_win_cnt, double *h_win_max, double *h_win_min,
                             int64_t *h_det_cnt, double *h_det_max, double *h_det_min);

/* ---------------------------------------------------------------------------
 * (4) Agglomerative clustering, spk_cluster_hi
 * (variant 1: spk-clustering.py:178-240, variant 2: spk-clustering2.py:173-222).
 * n_problems independent problems (files); problem p owns the records
 * [h_seg_off[p], h_seg_off[p+1]) of d_stats (read only).  Per problem:
 *   h_n_merges[p]; merge m of problem p at index h_seg_off[p] + m of
 *   h_merge_a / h_merge_b (compacted indices at the time of the merge, a < b)
 *   and h_merge_d (the minimum that triggered it);
 *   h_stat_max[p], h_stat_min[p]: variant 1 = running max / min over every
 *   finite distance evaluated (NaN when never updated from the reference's
 *   initial 0 / maxint); variant 2 = max / min of the final matrix.
 * The minimum and its position are numpy's distances.min() / distances.argmin(): the first
 * occurrence in row-major order; with a NaN present the minimum is NaN and the position the
 * first NaN.  -0.0 and +0.0 are equal, as to numpy: the first of them wins whatever its sign,
 * and a zero minimum comes back as +0.0 in h_merge_d (and as variant 2's h_stat_min, which is
 * that minimum; its h_stat_max is a plain fp64 maximum and keeps the sign of the zero it finds).
 * A forced merge (max_spk) of variant 2 whose minimum is +inf lands, like numpy's argmin, on the
 * first +inf in row-major order, the diagonal of the first alive row: the call fails as a
 * degenerate merge (variant 1's diagonal, 2^63, is below +inf: it ends the same way).
 */
/* Launch shape of the merge loop.  MONO: one launch, one workgroup per problem, the whole
 * loop inside it (many files per call).  WIDE: one launch per merge, its log-det work spread
 * over all CUs (one long file).  AUTO: WIDE up to 64 problems, MONO above.  Results are
 * identical.  MONO with a problem of more than 38 396 records (its ids outgrow the LDS) runs
 * WIDE instead.  WIDE refuses a problem of more than 16 384 records with SPKD_EINVAL before
 * any work, as every shape does one of more than 65 536. */
enum { SPKD_AHC_AUTO = 0, SPKD_AHC_MONO = 1, SPKD_AHC_WIDE = 2 };

typedef struct {
    int32_t variant;     /* 1 or 2 */
    int32_t kind;        /* spkd_kind */
    int32_t max_spk;     /* -ms */
    int32_t path;        /* SPKD_AHC_AUTO / _MONO / _WIDE */
    double lambdac;
    double threshold;
} spkd_ahc_params;

spkd_status spkd_ahc(spkd_ctx *ctx, const double *d_stats, const int64_t *h_seg_off,
                     int64_t n_problems, const spkd_ahc_params *params,
                     int32_t *h_n_merges, int32_t *h_merge_a, int32_t *h_merge_b,
                     double *h_merge_d, double *h_stat_max, double *h_stat_min);

/* Head and rest of a MONO call that computes its matrices in full (spkd_ahc, spkd_ahc_fused; not
 * SPKD_KL2_PINV): the K largest problems (ties by index) get their matrices first and run their
 * merge loops on a side stream of the context, beside the matrices of the others; the call still
 * returns with all of its work finished, whatever the status.  Results do not depend on K.
 * SPKD_AHC_HEAD in the environment, read when the context is created: unset or -1 = the rule
 * below decides, 0 = one launch of either kernel, k = the k largest (at most all).
 * With K > 0, SPKD_T_MATRIX and SPKD_T_AHC are spans (first start to last end of the two
 * launches of either kernel) that overlap.
 * spkd_ahc_head_rule: the K in 0 .. 32 that the rule gives for these problem sizes (host only;
 * -1: bad argument), a multiple of 32 (whole rounds of the shader engines: DESIGN.md par. 5),
 * so 0 or 32; 0 for fewer than 16 problems, and where the predicted saving is under 1 %.
 * spkd_last_ahc_head: the K of the context's most recent spkd_ahc / _matrix / _fused call. */
int64_t spkd_ahc_head_rule(const int64_t *h_seg_off, int64_t n_problems);
spkd_status spkd_last_ahc_head(spkd_ctx *ctx, int64_t *k);

/* spkd_ahc for ONE problem of n records whose initial n x n matrix the caller supplies
 * (d_matrix, device, in exactly the form spkd_ahc would have computed: see
 * spkd_distance_rows): the merge loop of spk-clustering.py:201-240 alone.  stat_max_in /
 * stat_min_in: variant 1's running max / min over the distances behind d_matrix (NaN: none);
 * ignored for variant 2.  Outputs as spkd_ahc's, problem 0. */
spkd_status spkd_ahc_matrix(spkd_ctx *ctx, const double *d_stats, int64_t n, const spkd_ahc_params *params,
                            const double *d_matrix, double stat_max_in, double stat_min_in,
                            int32_t *h_n_merges, int32_t *h_merge_a, int32_t *h_merge_b,
                            double *h_merge_d, double *h_stat_max, double *h_stat_min);

/* spkd_ahc for the lines of a spkd_gw_batch, in ONE call bracket: problem p owns the lines
 * [h_seg_off[p], h_seg_off[p+1]); line i's record is d_records[d_line_index[i]] (the fused
 * detector's buffer of n_records records and the view's d_index: what spkd_gather_stats used to
 * copy into segment order is read in place by the kernel that builds the clustering stage's
 * working copies), except for the n_redo lines of the redo list, whose records are computed
 * from the frames [h_redo_begin[k], h_redo_end[k]) first (the kernels of spkd_set_stats) --
 * the same records, so the same merges, as spkd_gather_stats / spkd_set_stats / spkd_ahc in
 * sequence (spk-clustering.py:263-292 read into 46-52, 88-94).  d_line_index is overwritten at
 * the redo lines.  A map entry outside [0, n_records) is SPKD_EOVERFLOW.
 * The outputs are pointers into pinned memory of the context, laid out as spkd_ahc's and
 * valid until the next spkd_ahc_fused; labels: the final 1-based cluster of every line
 * (spkd_labels_from_merges_batch of the merge log). */
spkd_status spkd_ahc_fused(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                           const double *d_records, int64_t n_records, int64_t *d_line_index,
                           const int64_t *h_seg_off, int64_t n_problems,
                           const int64_t *h_redo_line, const int64_t *h_redo_begin,
                           const int64_t *h_redo_end, int64_t n_redo,
                           const spkd_ahc_params *params,
                           const int32_t **h_n_merges, const int32_t **h_merge_a,
                           const int32_t **h_merge_b, const double **h_merge_d,
                           const int32_t **h_labels);

/* ---------------------------------------------------------------------------
 * (6) Feature front-end: what `feacat -c fconfig.cfg -H --raw-output x.wav` computes for the
 * reference (spk-diarization2.py:98-100; external AaltoASR C++, not in the reference tree)
 * with the module chain of fconfig.cfg:1-101: pre-emphasis, 400-sample Hamming windows at
 * 125 frames/s (window_width 256, the VAD models' .cfg, is built too: zero-padded to the
 * same 512-point transform), magnitude spectrum, mel filterbank + log, DCT (12 cepstra) and log power,
 * mean subtraction over +-75 frames, deltas and delta-deltas, normalization, 39x39
 * transform.  PARITY UNPINNED: feacat is not available, the semantics the configuration
 * file leaves open are documented choices (oracle/mfcc_numpy.py).
 * d_pcm: n_samples 16-bit mono samples in device memory; the caller passes the tables
 * (host): mel filterbank [21][257], DCT [12][21], mean[39], scale[39], transform[39][39].
 * d_features receives floor(n_samples / hop) frames of 39 floats (*h_n_frames).
 * Accepted parameters (anything else is SPKD_EINVAL before any device work):
 *   window_width 400 or 256, n_fft 512, n_mel 21, n_cep 12; frame_rate > 0 dividing sample_rate;
 *   cms_left >= 0, cms_right >= 0 (0, 0: every frame is its own mean, the mean-subtracted block
 *     is 0), cms_left + cms_right <= SPKD_MFCC_CMS_MAX: the post stage keeps the static rows of a
 *     tile of SPKD_MFCC_POST_TILE frames, its halo of SPKD_MFCC_POST_HALO to either side and the
 *     mean window in LDS, and
 *       4 * (13 * (3 * (TILE + 2 * HALO) + cms_left + cms_right) + 39 * TILE + 39 * 39)
 *     bytes must not exceed SPKD_MFCC_POST_LDS;
 *   delta_width[0], delta_width[1] each 1 or 2; delta_norm[0], delta_norm[1] > 0 (a NaN is refused).
 * Borders, for a file of T frames, T >= 1 (there is no lower limit; T = 0 writes nothing):
 *   a sample index outside [0, n_samples) is the nearest sample of the file, the predecessor of
 *     sample 0 is sample 0; a file shorter than a window has both ends of every window clamped;
 *   the mean of frame t is over the frames max(t - cms_left, 0) .. min(t + cms_right, T - 1) and
 *     divides by their count;
 *   d[t] = sum_{k=1..width} k (x[min(t + k, T - 1)] - x[max(t - k, 0)]) / norm, in both delta
 *     stages, the second over the first's d[0 .. T): for T below the reach of the deltas
 *     (T <= delta_width[0] + delta_width[1]) both clamps act on every frame, and T = 1 gives
 *     deltas and delta-deltas of exactly 0. */
typedef struct {
    int32_t sample_rate, frame_rate, window_width, n_fft, n_mel, n_cep;
    int32_t cms_left, cms_right;
    int32_t delta_width[2];
    float pre_emph;
    float delta_norm[2];
} spkd_mfcc_params;
#define SPKD_MFCC_POST_TILE 128
#define SPKD_MFCC_POST_HALO 4
#define SPKD_MFCC_POST_LDS 61440
#define SPKD_MFCC_CMS_MAX 272
spkd_status spkd_mfcc(spkd_ctx *ctx, const int16_t *d_pcm, int64_t n_samples,
                      const spkd_mfcc_params *params, const float *h_melfb, const float *h_dct,
                      const float *h_mean, const float *h_scale, const float *h_transform,
                      float *d_features, int64_t *h_n_frames);

/* The front-end for a whole batch of files: one table upload, one launch for the static stage of
 * every file and one for the post stage (mean subtraction to transform), one wait at the end,
 * whatever n_files is.  spkd_mfcc is this call with one file.
 * Layout: file f owns the samples d_pcm[h_sample_off[f] .. h_sample_off[f+1]) (h_sample_off[0] = 0,
 * non-decreasing; a file may be empty) and has T_f = n_f / hop frames, as spkd_mfcc counts them;
 * h_frame_off (out, n_files + 1 entries) is the running sum of T_f, and file f's features are the
 * rows [h_frame_off[f], h_frame_off[f+1]) of d_features, 39 floats each.  The sample offsets need
 * not be multiples of the hop: frame t of file f is centred on sample h_sample_off[f] + t * hop.
 * Borders: every rule of spkd_mfcc holds per file -- sample indices clamp to the file's own
 * samples, the mean is over the file's existing frames of [t - left, t + right], delta indices
 * clamp to [0, T_f) -- and a workgroup's tile of frames never crosses a file boundary, so nothing
 * of a neighbouring file enters a file's features: for every file the output equals spkd_mfcc's
 * for that file alone to the bit, for both window widths.
 * Refusals (SPKD_EINVAL before any device work): spkd_mfcc's parameter checks, n_files < 0, a
 * null h_sample_off / h_frame_off, offsets that do not start at 0 or decrease; null device
 * pointers only when there is a frame.  No file, or no frame in any: SPKD_OK, h_frame_off
 * filled, nothing launched.
 * Device scratch held by the context: the static rows, 52 bytes per frame of the batch.
 * Timers: SPKD_T_MFCC_STATIC, SPKD_T_MFCC_POST. */
spkd_status spkd_mfcc_batch(spkd_ctx *ctx, const int16_t *d_pcm, int64_t n_files,
                            const int64_t *h_sample_off /* [n_files + 1] */,
                            const spkd_mfcc_params *params, const float *h_melfb, const float *h_dct,
                            const float *h_mean, const float *h_scale, const float *h_transform,
                            float *d_features, int64_t *h_frame_off /* out [n_files + 1] */);

/* ---------------------------------------------------------------------------
 * (6b) Sample-rate conversion and downmix of a batch's audio: what `ffmpeg -i x -ar 16000 -ac 1`
 * does for the reference in front of everything else (spk-diarization2.py:83; an external program,
 * not in the reference tree).  One launch (k_resample) serves every file of the batch, whatever
 * mixture of rates and channel counts it holds, with one wait at the end; the output lies exactly
 * as spkd_mfcc_batch reads it.  PARITY UNPINNED: ffmpeg is not available, its resampler's filter
 * is not restated; the filter below is a documented choice (tests/resample_numpy.py restates it).
 *
 * The filter is designed on the host and handed over as a table, as the mel and DCT tables of
 * spkd_mfcc are.  For a conversion rate_in -> rate_out with g = gcd: up = L = rate_out / g,
 * down = M = rate_in / g, r = min(1, L / M), half_taps = ceil(16 / r), fc = 0.92 r, and for
 * phase p in [0, L), tap k in [-half + 1, half]:  t = k - p / L,
 *   h[p][k] = fc sinc(fc t) I0(9 sqrt(1 - (t / half)^2)) / I0(9)     (sinc(x) = sin(pi x) / (pi x)),
 * every row divided by its own sum (DC gain 1 at every phase): a Kaiser window (beta = 9) over 16
 * zero crossings to either side, half-amplitude point at 0.92 of the lower Nyquist frequency.  The
 * table is float32 [L][2 half_taps], row p at h_taps[taps_off + p * 2 * half_taps], tap k at
 * column k + half_taps - 1.  The call takes any table of that shape: it checks the shape, not the
 * design.
 *
 * Layout: file f owns the interleaved int16 elements d_in[h_in_off[f] .. h_in_off[f+1]) (h_in_off[0]
 * = 0, non-decreasing; a file may be empty; offsets of any parity), has h_channels[f] channels
 * (the span is a multiple of it), n_in = span / channels sample frames, and the conversion
 * h_convs[h_conv[f]].  s[j] is the exact integer sum of the channels of frame j, 0 for j outside
 * [0, n_in): zero padding per file, nothing of a neighbouring file enters (a workgroup's tile of
 * SPKD_RESAMPLE_TILE output samples never crosses a file).
 *   identity (up == down == 1, half_taps == 0):  n_out = n_in,  y[n] = rint((double)s[n] / channels);
 *   filtered:  n_out = ceil(n_in up / down) (every output instant inside the input's span); for
 *     output n:  i = n down div up,  p = n down mod up,
 *     acc = sum_k (double)h[p][k] s[i + k]   in fp64, k ascending,    y[n] = rint(acc / channels);
 * rint rounds half to even, the division is one correctly rounded fp64 division; y is saturated
 * to [-32768, 32767] (upsampled full-scale noise does overshoot) and stored as int16.  fp64
 * accumulation keeps any two evaluations within about 2 half 2^-53 sum |h||s| ~ 2e-8 of each other,
 * so the int16 result is the same almost everywhere whoever computes it.
 * h_out_off (out, n_files + 1 entries) is the running sum of n_out; file f's mono samples are
 * d_out[h_out_off[f] .. h_out_off[f+1]).
 * Refusals (SPKD_EINVAL before any device work): n_files < 0 or n_conv < 0; a null host array;
 * offsets that do not start at 0 or decrease; a span that is no multiple of the file's channel
 * count; a channel count outside [1, SPKD_RESAMPLE_MAX_CH]; a conversion index out of range; up or
 * down outside [1, SPKD_RESAMPLE_MAX_TERM]; gcd(up, down) != 1; half_taps outside [0,
 * SPKD_RESAMPLE_MAX_HALF]; half_taps == 0 unless up == down == 1, and the converse; taps_off < 0;
 * a table of more than SPKD_RESAMPLE_MAX_TAPS floats; a tile whose input span,
 * ceil(SPKD_RESAMPLE_TILE down / up) + 2 half_taps frames, exceeds SPKD_RESAMPLE_MAX_SPAN (the
 * span is kept in LDS; a designed filter of at most SPKD_RESAMPLE_MAX_HALF never does); null tables
 * with a filtered conversion; null device pointers only when there is a sample.  No file, or no
 * sample in any: SPKD_OK, h_out_off filled, nothing launched.
 * Timer: SPKD_T_RESAMPLE. */
typedef struct { int32_t up, down, half_taps; int64_t taps_off; } spkd_resample_conv;
#define SPKD_RESAMPLE_TILE 2048
#define SPKD_RESAMPLE_MAX_CH 8
#define SPKD_RESAMPLE_MAX_HALF 256
#define SPKD_RESAMPLE_MAX_TERM 1048576
#define SPKD_RESAMPLE_MAX_TAPS 4194304
#define SPKD_RESAMPLE_MAX_SPAN 33281
spkd_status spkd_resample_batch(spkd_ctx *ctx, const int16_t *d_in, int64_t n_files,
                                const int64_t *h_in_off /* [n_files + 1], int16 elements */,
                                const int32_t *h_channels /* [n_files] */,
                                const int32_t *h_conv /* [n_files] -> h_convs */, int32_t n_conv,
                                const spkd_resample_conv *h_convs, const float *h_taps /* all tables, concatenated */,
                                int16_t *d_out, int64_t *h_out_off /* out [n_files + 1] */);

/* ---------------------------------------------------------------------------
 * (6b2) Delay-and-sum beamforming of multi-microphone recordings, in front of the resampler: the
 * channels of a table-top array carry the same voice at different delays, so their plain average
 * (what (6b) forms, and `ffmpeg -ac 1`) comb-filters it.  Three calls, one per stage: the GCC-PHAT
 * correlation of every channel against a reference channel and its best lags per analysis step
 * (spkd_bf_gcc), a Viterbi over the steps that picks one lag per step and channel (spkd_bf_track),
 * and the sum of the channels at those lags (spkd_bf_sum).  The stages are separate so that each can
 * be checked exactly from the previous one's output, and because the delays are worth having on
 * their own (a known array geometry skips stage 1).  PARITY UNPINNED: the reference has no such
 * stage; BeamformIt, the usual program of this scheme, is not available and not restated, and no
 * parity with it or any other beamformer is claimed.  tests/beamform_numpy.py restates all three
 * stages.  Opt-in: nothing else in this header calls them.
 *
 * Layout.  A file has C channels of interleaved int16, n sample frames, and a geometry (hop H,
 * window W, max_lag D) in samples.  The transform length is fixed: SPKD_BF_NFFT = 8192.  Geometry
 * limits: 1 <= H <= SPKD_BF_MAX_HOP = 2^20; 1 <= W; 0 <= D; W + D <= 8192, so every lag in [-D, D]
 * of the circular correlation is alias-free.  Files and geometries follow spkd_resample_batch's
 * conventions: file f owns the int16 elements d_in[h_in_off[f] .. h_in_off[f+1]) (h_in_off[0] = 0,
 * non-decreasing, offsets of any parity, the span a multiple of h_channels[f] in [1, 8]) and has
 * the geometry h_geoms[h_geom[f]].
 *
 * Steps and reference channel.  The file has T = 1 step if n <= W, else T = (n - W) div H + 1.
 * Step t reads frames [t H, t H + W), with zeros beyond the file.  Nothing of a neighbouring file
 * ever enters.  C = 1 gives T = 0: the file is copied through.  A requested reference channel
 * ref >= 0 is taken as given.  ref = -1 picks the channel with the largest exact int64 sum of
 * squares, and a tie goes to the lowest index.  The sum fits: 10 h at 96 kHz full scale is
 * 3.7e18.
 *
 * Stage 1, correlation.  For each step and each channel c != ref: a is the step's reference window
 * and b is channel c's window, as float32 zero-padded to 8192 (the int16 samples are exact in
 * float32).  A, B are their forward DFTs (e^{-2 pi i k n / N}).  P_k = B_k conj(A_k).
 * G_k = P_k / |P_k| where |P_k| > 0, else 0.  r[m] = Re (1/N) sum_k G_k e^{+2 pi i k m / N}, and
 * v[d] = r[d mod N] for d in [-D, D], as float32.  With x_c[n] = x_ref[n - d] this puts the peak at
 * +d.  (The device forms both spectra from one float32 transform of a + i b and treats a window
 * that is all zero as the exact zero spectrum it has; where one channel is far quieter than the
 * other, its spectrum carries the louder one's rounding, about 1e-7 of it.)
 * A lag is a candidate if both of these hold:  v[d] > v[d-1], or d = -D;  v[d] >= v[d+1], or d = D.
 * The candidates are ranked by value descending, and ties go to the lower lag.  The first
 * SPKD_BF_NBEST = 4 are kept as (lag int32, value float32).  Missing slots carry slot 0's lag and
 * value -INFINITY.  The reference channel's own entry is (0, 1.0f) and three absent slots (lag 0),
 * and its row of the curve is 1 at lag 0 and 0 elsewhere, by definition, not by a transform.
 * Digital silence gives v = 0 everywhere, hence the single candidate (-D, 0).
 *
 * Stage 2, tracking, per file and channel, serially over the steps, with the options n_best in
 * [1, 4] (only the first n_best slots are used; the others count as absent), min_peak (float32),
 * jump_penalty lambda (double, >= 0, finite) and jump_cap (int32, >= 0).  A step is reliable if its
 * slot-0 value is >= min_peak.  An unreliable step takes its lags from a reliable step of the same
 * channel: the nearest earlier one, if there is one; else the nearest later one; else the single
 * candidate lag 0, if the channel has none at all.  The present slots of a filled step get value 0,
 * and absent slots stay -INFINITY.  Viterbi over the slots:
 *   S[0][k] = (double)val[0][k];
 *   S[t][k] = max_j (S[t-1][j] - lambda (double)min(|lag[t][k] - lag[t-1][j]|, cap)) + (double)val[t][k]:
 *   one rounded multiply, one rounded subtract, one rounded add, in that order, with no contraction
 *   into an FMA; ties in j go to the lower j.
 * The end state is the best k, with ties to the lower k; then backtrack.  The output is
 * delay[t][c], int32.  Given the same candidates, a host restatement reproduces this to the bit.
 *
 * Stage 3, sum.  The anchors are a_t = t H + W div 2.  For output sample n the pair (t0, t1, j) is:
 *   n < a_0: (0, 0, 0);   n >= a_{T-1}: (T-1, T-1, 0);
 *   else: t0 = (n - a_0) div H, t1 = t0 + 1, j = (n - a_0) mod H.
 * num = sum_c [(H - j) x_c[n + delay[t0][c]] + j x_c[n + delay[t1][c]]] in int64; x_c outside
 * [0, n) is 0.  y[n] = rint((double)num / (double)(C H)), saturated to int16: one correctly rounded
 * division with half to even, as (6b) rounds.  The linear cross-fade between neighbouring steps'
 * delays is what keeps a delay change from clicking.  num is exact, so the stage is bit-exact
 * whoever computes it.
 *
 * spkd_bf_gcc: h_ref[n_files] is the requested reference channel of each file, -1 to pick.  Writes
 *   d_ref int32 [n_files]; d_lag int32 and d_val float32 at cand_off[f] + ((t C + c) 4 + k), with
 *   cand_off the running sum of 4 T C; h_step_off[n_files + 1], the running sum of T.  An optional
 *   d_curve (null in production) receives every v as float32 [T][C][2 D + 1] per file, file f's at
 *   h_curve_off[f] (out, n_files + 1 entries, the running sum of T C (2 D + 1); may be null with a
 *   null d_curve).
 *   Refusals (SPKD_EINVAL before any device work): n_files < 0 or n_geom < 0; a null host array;
 *   offsets that do not start at 0 or decrease; a channel count outside [1, 8]; a span that is no
 *   multiple of the file's channel count; a geometry index out of range; a hop outside
 *   [1, SPKD_BF_MAX_HOP]; a window below 1; a negative max_lag; window + max_lag above
 *   SPKD_BF_NFFT; a reference channel outside [-1, channels); more than 2^31 - 1 steps times
 *   channels; null device pointers only when there is a sample.  No file, or no sample in any:
 *   SPKD_OK, the host offsets filled, nothing launched, the device arrays untouched.
 *   Timer: SPKD_T_BF_GCC (all launches of the call).
 * spkd_bf_track: h_step_off and h_channels as above (the candidates lie as spkd_bf_gcc leaves
 *   them), the options by value; d_delay int32 at delay_off[f] + t C + c, delay_off the running sum
 *   of T C.  Refusals: n_files < 0; a null host array; step offsets that do not start at 0 or
 *   decrease; a channel count outside [1, 8]; n_best outside [1, 4]; a min_peak that is not a
 *   number; a jump_penalty that is negative or not finite; a negative jump_cap; null device pointers
 *   only when there is a step.  No step: SPKD_OK, nothing launched.  Device scratch held by the
 *   context: one byte per step and channel.  Timer: SPKD_T_BF_TRACK.
 * spkd_bf_sum: the audio and geometries as for spkd_bf_gcc, d_delay as spkd_bf_track leaves it.
 *   Mono int16 out at the file's own rate, n samples per file, laid out as spkd_resample_batch
 *   reads a one-channel file; h_out_off (out, n_files + 1 entries) is their running sum.  Delays
 *   are not limited to [-D, D]: a sample they point outside the file is 0.  Refusals: those of
 *   spkd_bf_gcc on files and geometries; a null h_out_off; null device pointers only when there is
 *   a sample.  No sample: SPKD_OK, h_out_off filled, nothing launched.  Timer: SPKD_T_BF_SUM. */
typedef struct { int32_t hop, window, max_lag; } spkd_bf_geom;
#define SPKD_BF_NFFT 8192
#define SPKD_BF_NBEST 4
#define SPKD_BF_MAX_HOP 1048576
spkd_status spkd_bf_gcc(spkd_ctx *ctx, const int16_t *d_in, int64_t n_files,
                        const int64_t *h_in_off /* [n_files + 1], int16 elements */,
                        const int32_t *h_channels /* [n_files] */,
                        const int32_t *h_geom /* [n_files] -> h_geoms */, int32_t n_geom,
                        const spkd_bf_geom *h_geoms, const int32_t *h_ref /* [n_files], -1: pick */,
                        int32_t *d_ref, int32_t *d_lag, float *d_val, float *d_curve /* or NULL */,
                        int64_t *h_step_off /* out [n_files + 1] */, int64_t *h_curve_off /* out [n_files + 1] */);
spkd_status spkd_bf_track(spkd_ctx *ctx, int64_t n_files, const int64_t *h_step_off /* [n_files + 1] */,
                          const int32_t *h_channels /* [n_files] */, const int32_t *d_lag, const float *d_val,
                          int32_t n_best, float min_peak, double jump_penalty, int32_t jump_cap,
                          int32_t *d_delay);
spkd_status spkd_bf_sum(spkd_ctx *ctx, const int16_t *d_in, int64_t n_files,
                        const int64_t *h_in_off /* [n_files + 1], int16 elements */,
                        const int32_t *h_channels /* [n_files] */,
                        const int32_t *h_geom /* [n_files] -> h_geoms */, int32_t n_geom,
                        const spkd_bf_geom *h_geoms, const int32_t *d_delay,
                        int16_t *d_out, int64_t *h_out_off /* out [n_files + 1] */);

/* ---------------------------------------------------------------------------
 * (6b3) The delay stream: the per-step delays of spkd_bf_track, kept for a whole batch, as a second
 * feature stream of the resegmentation stage (section 8).  A delay is where the talker sits; the
 * stream's statistics are integers and exact, its models one Gaussian per (speaker, channel), and
 * their weighted log-likelihood is added to the score matrix every decoder of section 8 reads.
 * PARITY: no reference counterpart; tests/tdoa_numpy.py restates every rule.
 *
 * The stream.  One device array of int32.  File f owns the entries [off_f, off_f + T_f C_f); entry
 *   off_f + t C_f + c is the tracked delay of step t on channel c, in input samples, |delay| <=
 *   SPKD_TDOA_MAX_DELAY, or SPKD_TDOA_NONE where the step is not reliable on that channel (the first
 *   candidate's value below min_peak, both float32).  A one-channel file has T = 0.
 * The file table.  SPKD_TDOA_FILE int64 per file, on the host: off (entries before the file), T, C,
 *   the reference channel, H (the step, in input samples), the input rate, the file's first frame in
 *   the batch's frame numbering, 0.
 * The step rule.  With hop and window the feature configuration's, in samples at rate_out, frame t
 *   of file f (file-local) belongs to the step
 *       min(T_f - 1, ((t * hop + window / 2) * rate_in_f) / (rate_out * H_f)),
 *   in 64-bit integers with truncating division: the step whose first sample is the last at or
 *   before the centre of the frame's window.  Stated once, in csrc/spkd_tdoa.hpp (tdoa_step), for the
 *   host tables and the kernels.  The bound: (t * hop + window / 2) * rate_in < 2^63 for every frame
 *   handed in, and T * rate_out * H < 2^63; a call that would pass either is refused.  A step is at
 *   least a frame long (H * rate_out >= hop * rate_in), so consecutive frames differ by at most one
 *   step; a file that breaks this is refused.
 *
 * spkd_tdoa_pack: d_out[i] = d_val[4 i] >= min_peak ? d_delay[i] : SPKD_TDOA_NONE for i < n; d_delay
 *   and d_val as spkd_bf_track read and wrote them, d_out the place of these entries in the stream.
 *   One lane per entry.  Refusals: n < 0, a min_peak that is not a number, a null or misaligned
 *   device pointer when n > 0.  Timer: SPKD_T_TDOA_PACK.
 * spkd_tdoa_stats: frame ranges [begin, end) in the batch's numbering, each with its file and its set,
 *   the sets ascending (what spkd_set_stats takes, and the file).  d_stats int64 [n_sets][8][3]:
 *   per channel (n, sum x, sum x^2) over the frames of the set's ranges whose step is reliable there;
 *   the reference channel and channels >= C stay 0, as do one-channel files.  The work is per step:
 *   the frames of a range in a step are one interval, whose length weighs the step; sums in the wave
 *   and in LDS, then one 64-bit integer atomic add per (set, channel, moment) and workgroup: exact,
 *   and the same bits in every run.  |x| <= 4096 keeps sum x^2 inside int64 for any n < 2^39; a set
 *   whose ranges hold 2^31 frames or more is refused.  A range may run past the file's last step
 *   (the clamp).  Refusals (SPKD_EINVAL before any device work): a bad file table (above), sets that
 *   descend or lie outside [0, n_sets), a file index out of range, a range that starts before its
 *   file's first frame or ends before it starts, null arrays.  Timer: SPKD_T_TDOA_STATS.
 * spkd_tdoa_models: per (speaker, channel) of d_stats: ok_c = n >= min_frames, mean = (double)sum x /
 *   (double)n, var = max((double)sum x^2 / (double)n - mean * mean, floor_f) with floor_f = (floor_s *
 *   rate_in)^2, every operation rounded on its own (no contraction).  d_models double
 *   [n_speakers][8][SPKD_TDOA_MODEL]: mean, var, 1 / (2 var), -1/2 log(2 pi var); a (speaker, channel)
 *   that is not ok_c, the reference channel and channels >= C hold (0, floor_f, 0, 0), which adds 0
 *   to a score.  h_spk_file: the file of every speaker, ascending; h_ok: the speakers' acoustic
 *   models.  A channel is live in a file iff it is ok_c for every speaker of the file whose h_ok is
 *   not 0; h_live [n_files] receives the bit mask (bit c: channel c), 0 for a one-channel file.
 *   Refusals: min_frames < 1, a floor_s that is not a finite number > 0, speakers' files that
 *   descend or lie outside [0, n_files), a bad file table, null arrays.  Timer: SPKD_T_TDOA_MODELS.
 * spkd_tdoa_score: the sequences and d_scores [sum len, n_cols] as spkd_gauss_loglik left them, each
 *   sequence with its file.  For every frame of every sequence and every column j < its model count
 *       scores[frame, j] = (float)((double)scores[frame, j] + weight * ll),
 *       ll = sum over c live in the file and reliable at step(frame), ascending, of
 *            -1/2 log(2 pi var) - (x - mean)^2 * (1 / (2 var)),
 *   in fp64, each operation rounded on its own.  An entry that is not finite (-inf, NaN) and the
 *   columns past the model count keep their bits; a file without a live channel and a one-channel
 *   file are not touched.  One workgroup per tile of SPKD_TDOA_TILE frames of a sequence: the tile's
 *   steps and the sequence's models go into LDS once, the entries are read and written in 16-byte
 *   pieces between the tile's first and last 16-byte border.  Refusals: n_cols outside [1, 16], a
 *   weight that is not finite and >= 0, a sequence's models outside [0, n_models) or more than n_cols,
 *   a live channel its file does not have, those of spkd_tdoa_stats on files and ranges.
 *   Timer: SPKD_T_TDOA_SCORE. */
#define SPKD_TDOA_NONE INT32_MIN
#define SPKD_TDOA_MAX_CH 8
#define SPKD_TDOA_MAX_DELAY 4096
#define SPKD_TDOA_FILE 8
#define SPKD_TDOA_MODEL 4
#define SPKD_TDOA_TILE 256
spkd_status spkd_tdoa_pack(spkd_ctx *ctx, const int32_t *d_delay, const float *d_val, float min_peak, int64_t n,
                           int32_t *d_out);
spkd_status spkd_tdoa_stats(spkd_ctx *ctx, const int32_t *d_stream, int64_t n_entries,
                            const int64_t *h_files /* [n_files][SPKD_TDOA_FILE] */, int64_t n_files,
                            int32_t hop, int32_t window, int32_t rate_out,
                            const int64_t *h_begin, const int64_t *h_end, const int32_t *h_file,
                            const int32_t *h_set, int64_t n_ranges, int64_t n_sets, int64_t *d_stats);
spkd_status spkd_tdoa_models(spkd_ctx *ctx, const int64_t *d_stats, int64_t n_speakers,
                             const int32_t *h_spk_file, const int32_t *h_ok, const int64_t *h_files,
                             int64_t n_files, int32_t min_frames, double floor_s, double *d_models,
                             int32_t *h_live /* out [n_files] */);
spkd_status spkd_tdoa_score(spkd_ctx *ctx, const int32_t *d_stream, int64_t n_entries,
                            const int64_t *h_files, int64_t n_files, int32_t hop, int32_t window,
                            int32_t rate_out, const double *d_models, int64_t n_models,
                            const int32_t *h_live, int64_t n_seq, const int64_t *h_seq_begin,
                            const int64_t *h_seq_end, const int32_t *h_seq_file, const int32_t *h_seq_model,
                            const int32_t *h_seq_n_models, int32_t n_cols, double weight, float *d_scores);

/* ---------------------------------------------------------------------------
 * (6b4) Seats from the delay stream: where the delays of a file change, a talker has moved or another one
 * speaks from another place.  Two calls on the exact integer records of spkd_tdoa_stats: the best cut of a
 * frame range (behind change detection) and an agglomerative chain over the records of a group of segments
 * (behind clustering).  Stated once in csrc/spkd_seat.hpp, for both kernels.
 * PARITY: no reference counterpart; tests/seat_numpy.py restates every rule.
 *
 * The statistic.  A record is int64 [8][3], per channel (n, sum x, sum x^2), in frames.  For a file
 *       w       = (double)(H * rate_out) / (double)(hop * rate_in)      (frames per step: an observation is a
 *                                                                        step, the sums are in frames only
 *                                                                        because ranges cut steps)
 *       floor_f = (floor_s * (double)rate_in)^2                          (as spkd_tdoa_models)
 *   and one channel of a record gives, every operation rounded on its own (no contraction), in this order,
 *       dn = (double)n;  mean = (double)sx / dn;  v = (double)sxx / dn - mean * mean;
 *       var = v > floor_f ? v : floor_f;  g = dn * log(var).
 *   For two records A and B of one file, channel c counts iff n_A,c >= min_frames and n_B,c >= min_frames;
 *   the reference channel and channels >= C never count.  Over the counted channels, ascending, from d = 0.0:
 *       t = g(A_c + B_c) - g(A_c);  t = t - g(B_c);  t = 0.5 * t;  t = t / w;     (A_c + B_c: exact integer sums)
 *       p = (double)(n_A,c + n_B,c) / w;  p = log(p);  p = lambdac * p;
 *       d = d + (t - p).
 *   Delta(A, B) = d, undefined when no channel counts.  Delta > threshold means two seats.  The earlier
 *   record (the left side of a cut, the lower position of a pair) is A.
 *
 * spkd_tdoa_cuts: the stream, the file table and the clock as spkd_tdoa_stats takes them; n_ranges frame
 *   ranges [begin, end) in the batch's numbering, each with its file.  The candidates of a range are the frames
 *   t in (begin, end) with step(t) != step(t - 1), t - begin >= min_piece and end - t >= min_piece; a
 *   candidate's value is Delta(record of [begin, t), record of [t, end)), the records weighted by frames
 *   exactly as spkd_tdoa_stats weighs a step; a range may run past the file's last step (the clamp).
 *   h_cut[r]: the candidate with the highest defined Delta, the lowest frame among equals, if that Delta >
 *   threshold, else -1.  h_delta[r]: that highest Delta, cut or not; NaN when no candidate has a defined one
 *   (a range inside one step, a one-channel file, an empty range).  A workgroup per range: totals first,
 *   then tiles of 256 steps staged in LDS, exact int64 prefix sums carried tile to tile, a lane per candidate,
 *   an arg-max with the tie rule.  No atomics; the bits do not depend on the other ranges of the call.
 *   Refusals (SPKD_EINVAL before any device work): every argument spkd_tdoa_stats refuses, a range of 2^31
 *   frames or more, min_piece < 1, min_frames < 1, a floor_s that is not finite and > 0, a lambdac that is
 *   not finite, a NaN threshold.  n_ranges = 0: SPKD_OK without a launch.  Timer: SPKD_T_TDOA_CUTS.
 * spkd_tdoa_split: problem p owns the records [h_off[p], h_off[p + 1]) of d_stats, int64 [n][8][3], and is of
 *   file h_prob_file[p] of the file table (the clock gives w).  A record is placed iff some channel of it that
 *   can count has n >= min_frames; unplaced records take no part.  A step looks over the live placed
 *   clusters of the problem for the pair a < b with the lowest defined Delta, the first in row-major order on
 *   a tie; the pair is merged iff not (Delta > threshold), otherwise the chain stops, as it does when no pair
 *   has a defined Delta.  A merge is record[a] += record[b] in exact integers, then pop(b): spkd_ahc's log
 *   convention, which spkd_labels_from_merges replays; only row and column a are computed again.  The log of
 *   problem p (a, b, Delta; up to n_p - 1 entries) starts at h_off[p], as spkd_ahc's does, and has
 *   h_n_merges[p] entries; h_placed [n]: 1 for a placed record.  d_stats is not modified.  One workgroup per
 *   problem, all problems in one launch; the matrix is n_p^2 doubles of device scratch, the per-row best
 *   waits in LDS.  The bits of a problem's log depend neither on the grid nor on the other problems.
 *   Limit: n_p <= SPKD_SEAT_MAX_N = 4096, above that SPKD_EINVAL.  Problems of 0 or 1 records: no merges.
 *   Refusals: a bad file table or clock, offsets that do not start at 0 or descend, a file index out of
 *   range, the four settings as above, null arrays.  n_problems = 0: SPKD_OK without a launch.
 *   Timer: SPKD_T_TDOA_SPLIT. */
#define SPKD_SEAT_MAX_N 4096
spkd_status spkd_tdoa_cuts(spkd_ctx *ctx, const int32_t *d_stream, int64_t n_entries,
                           const int64_t *h_files /* [n_files][SPKD_TDOA_FILE] */, int64_t n_files,
                           int32_t hop, int32_t window, int32_t rate_out,
                           const int64_t *h_begin, const int64_t *h_end, const int32_t *h_file,
                           int64_t n_ranges, int64_t min_piece, int32_t min_frames, double floor_s,
                           double lambdac, double threshold, int64_t *h_cut /* out [n_ranges] */,
                           double *h_delta /* out [n_ranges] */);
spkd_status spkd_tdoa_split(spkd_ctx *ctx, const int64_t *d_stats, int64_t n_problems,
                            const int64_t *h_off /* [n_problems + 1] */, const int32_t *h_prob_file,
                            const int64_t *h_files, int64_t n_files, int32_t hop, int32_t window,
                            int32_t rate_out, int32_t min_frames, double floor_s, double lambdac,
                            double threshold, int32_t *h_merge_a, int32_t *h_merge_b, double *h_merge_d,
                            int32_t *h_n_merges /* out [n_problems] */, int32_t *h_placed /* out [n] */);

/* ---------------------------------------------------------------------------
 * (6b5) Overlapped speech from the delay stream: when two talkers at two seats speak in one step, the tracked
 * delay is one talker's seat and the runner-up among the step's GCC-PHAT candidates is the other's.  A second
 * stream keeps the runner-up, and one call names, per step, the pair of speakers whose delay models the two lags
 * fit on enough channels.  Opt-in; stated once in csrc/spkd_overlap.hpp.
 * PARITY: no reference counterpart; tests/overlap_numpy.py restates every rule.
 *
 * The runner-up stream.  int32 with the layout of the delay stream (6b3): the same offsets, the same file table,
 *   SPKD_TDOA_NONE where a step has no runner-up on a channel.
 * spkd_tdoa_second: for entry i < n, with d_delay[i], d_lag[4 i + k] and d_val[4 i + k] as spkd_bf_track read and
 *   wrote them: if d_val[4 i] < min_peak (the step is not reliable) d_out[i] = SPKD_TDOA_NONE.  Else the slots
 *   k = 0 .. n_best - 1 are walked in order; the first with a finite value and |d_lag[4 i + k] - d_delay[i]| > guard
 *   is the runner-up, and d_out[i] is its lag if its value >= min_second (float32), SPKD_TDOA_NONE if not, and
 *   SPKD_TDOA_NONE when no slot qualifies.  The reference channel's entry holds one finite slot, at its own delay
 *   (spkd_bf_gcc), so it is SPKD_TDOA_NONE by the same walk.  One lane per entry.  Refusals: n < 0, n_best outside
 *   [1, 4], guard < 0, a min_peak or min_second that is not a number, a null or misaligned device pointer when
 *   n > 0.  Timer: SPKD_T_TDOA_SECOND.
 * spkd_tdoa_overlap: both streams and the file table as spkd_tdoa_stats takes them; d_models and h_live as
 *   spkd_tdoa_models left them; h_spk_off [n_files + 1]: the speakers of file f are the consecutive models
 *   [h_spk_off[f], h_spk_off[f + 1]), at most SPKD_OVERLAP_MAX_SPK.  d_pair: int32 [sum of T_f][2], the steps of the
 *   files one after the other.
 *   Near: a lag x is near speaker j on channel c iff ((double)x - mean) * ((double)x - mean) * inv2var <= gate, with
 *   mean and inv2var = 1 / (2 var) the model's, every operation rounded on its own (no contraction).
 *   Agreement: channel c agrees with the pair j < k at step t iff c is live in the file, is not the reference
 *   channel, the tracked delay p and the runner-up q are both present, and one of {p, q} is near j while the other
 *   is near k, in either assignment.
 *   The raw pair of a step is the (j, k) with the most agreeing channels n_jk, the lexicographically smallest on a
 *   tie, if n_jk >= min(min_channels, live non-reference channels of the file) and n_jk >= 1; else (-1, -1).  A
 *   file with no live channel, with fewer than two speakers or with one channel yields only (-1, -1).
 *   The run filter: a step keeps its raw pair iff it lies in a run of at least min_steps consecutive steps of its
 *   file with the same raw pair; runs never cross files.  j and k count from the file's first model.
 *   Two launches: the match (a workgroup per tile of SPKD_TDOA_TILE steps of one file, a lane per step, the file's
 *   models staged in LDS once, per channel two 16-bit speaker masks from which the pairs are counted), then the
 *   run filter (a lane per step, at most min_steps - 1 neighbours read on each side).  No atomics; the bits of a
 *   file's steps do not depend on the other files of the call.
 *   Refusals (SPKD_EINVAL before any device work): those of spkd_tdoa_stats on the file table and the clock,
 *   speaker offsets that do not start at 0 or that descend, more than 16 speakers in a file, a live channel a
 *   file does not have, a gate that is not finite and > 0, min_channels < 1, min_steps outside [1,
 *   SPKD_OVERLAP_MAX_RUN], null arrays.  No step: SPKD_OK with nothing launched.  Timer: SPKD_T_TDOA_OVERLAP, over
 *   both launches. */
#define SPKD_OVERLAP_MAX_SPK 16
#define SPKD_OVERLAP_MAX_RUN 64
spkd_status spkd_tdoa_second(spkd_ctx *ctx, const int32_t *d_delay, const int32_t *d_lag, const float *d_val,
                             int32_t n_best, float min_peak, float min_second, int32_t guard, int64_t n,
                             int32_t *d_out);
spkd_status spkd_tdoa_overlap(spkd_ctx *ctx, const int32_t *d_stream, int64_t n_entries,
                              const int64_t *h_files /* [n_files][SPKD_TDOA_FILE] */, int64_t n_files,
                              int32_t hop, int32_t window, int32_t rate_out, const int32_t *d_second,
                              const double *d_models, const int32_t *h_live /* [n_files] */,
                              const int64_t *h_spk_off /* [n_files + 1] */, double gate, int32_t min_channels,
                              int32_t min_steps, int32_t *d_pair /* out [sum T][2] */);

/* ---------------------------------------------------------------------------
 * (6c) The seed stage of a speech / non-speech detector trained on the recording itself: frame
 * energies from the samples and, per file, two order statistics of them with the runs of frames at
 * or beyond each -- the quietest frames seed a non-speech model, the loudest a speech model
 * (spkd_gmm_train on the runs, spkd_gmm_loglik_seq and spkd_mindur_viterbi_batch behind it:
 * self_vad.py).  It stands where the reference loads a VAD model (generate_exp.py:94-97).
 * PARITY: no reference counterpart; tests/self_vad_numpy.py restates both calls in numpy.
 *
 * spkd_frame_energy_batch: the samples lie as frontend.upload_batch leaves them and spkd_mfcc_batch
 *   reads them: file f owns d_pcm[h_sample_off[f] .. h_sample_off[f+1]) (h_sample_off[0] = 0,
 *   non-decreasing; a file may be empty; offsets of any parity) and has T_f = n_f / hop frames, the
 *   frame clock of spkd_mfcc_batch: h_frame_off (out, n_files + 1 entries) equals that call's.  Frame t
 *   of a file covers the file's samples t hop .. t hop + window - 1; a sample past the file's end
 *   counts as 0 and is never read from the neighbouring file (a workgroup's tile never crosses a file).
 *     d_energy[h_frame_off[f] + t] = window * sum s^2 - (sum s)^2           as int64
 *   which is window^2 times the frame's variance: a DC offset cancels.  Limits: 1 <= hop <= window <=
 *   SPKD_ENERGY_MAX_WINDOW = 4096.  With these |sum s| <= 2^12 2^15 = 2^27 and sum s^2 <= 2^12 2^30 =
 *   2^42, so both terms are at most 2^54 and the value lies in [0, 2^54] (below 2^55): every
 *   operation is an exact integer operation and no rounding occurs anywhere.  The value does not
 *   depend on the grid, on the other files or on their order.
 *   One launch for the batch and one wait.  A workgroup takes the frames whose hops fill
 *   SPKD_ENERGY_TILE samples; each sample is added once, into the sums of its 16-byte cell, the cells
 *   are scanned in LDS and a frame is the difference of two prefixes, so neighbouring frames share
 *   their common pieces.  The batch is read once from memory; the window - hop samples two tiles share
 *   are read a second time through L2.
 *   SPKD_EINVAL before any device work: hop or window outside the limits, n_files < 0, a null
 *   h_sample_off / h_frame_off, offsets that do not start at 0 or decrease; null or misaligned device
 *   pointers only when there is a frame.  No file, or no frame in any: SPKD_OK, h_frame_off filled,
 *   nothing launched.  Timer: SPKD_T_FRAME_ENERGY.
 *
 * spkd_energy_seeds: file f owns the energies d_energy[h_frame_off[f] .. h_frame_off[f+1]) (any int64
 *   values >= 0), T_f of them.  h_lo[f] is the h_k_low[f]-th smallest of them (1-based), h_hi[f] the
 *   h_k_high[f]-th largest; the selection is on the integer keys, so it is exact.  h_seeded[f] = 1 when
 *   both k are >= 1, both are <= T_f, and lo < hi; otherwise 0, which is no error: the file gets no
 *   runs (a k outside [1, T_f] leaves lo = hi = 0).  For a seeded file class 0 is every maximal run of
 *   consecutive frames with E <= lo, class 1 every maximal run with E >= hi; ties at a threshold are
 *   all taken, and a run never crosses a file.
 *   Out, in pinned memory of the context, valid until its next spkd_energy_seeds (the way
 *   spkd_vad_viterbi_batch hands back its tokens): (*h_run_off)[2 n_files + 1], the runs of file f and
 *   class c at [run_off[2 f + c], run_off[2 f + c + 1]) of *h_run_begin / *h_run_end, absolute frame
 *   numbers of the batch [begin, end), ascending -- what spkd_gmm_train takes as (h_set_off,
 *   h_range_begin, h_range_end) with speaker 2 f + c when every file is seeded (it refuses a set
 *   without a range: the caller leaves the unseeded files' sets out).
 *   A workgroup per file: eight passes of a 256-bin histogram in LDS find both order statistics at
 *   once and the runs are counted; after one wait for the counts a second launch flags, scans and
 *   compacts the runs to their exact offsets: run memory is 16 bytes a run, not per frame.
 *   SPKD_EINVAL before any device work: a null output or host array, n_files < 0, offsets that do not
 *   start at 0 or decrease, a file of more than 2^31 - 1 frames; a null or misaligned d_energy only
 *   when there is a frame.  n_files = 0: SPKD_OK, run_off = {0}.  Timer: SPKD_T_ENERGY_SEEDS (both
 *   launches and the wait between them). */
#define SPKD_ENERGY_MAX_WINDOW 4096
#define SPKD_ENERGY_TILE 16384
spkd_status spkd_frame_energy_batch(spkd_ctx *ctx, const int16_t *d_pcm,
                                    const int64_t *h_sample_off /* [n_files + 1] */, int64_t n_files,
                                    int32_t hop, int32_t window, int64_t *d_energy,
                                    int64_t *h_frame_off /* out [n_files + 1] */);
spkd_status spkd_energy_seeds(spkd_ctx *ctx, const int64_t *d_energy,
                              const int64_t *h_frame_off /* [n_files + 1] */, int64_t n_files,
                              const int64_t *h_k_low, const int64_t *h_k_high /* [n_files] each */,
                              int64_t *h_lo, int64_t *h_hi, int32_t *h_seeded /* [n_files] each */,
                              const int64_t **h_run_off, const int64_t **h_run_begin,
                              const int64_t **h_run_end);

/* ---------------------------------------------------------------------------
 * (7) Speech / non-speech frame scoring: the per-frame state log-likelihoods that AaltoASR's
 * `phone_probs` writes for generate_exp.py (generate_exp.py:94-97; external C++, not in the
 * reference tree) from a diagonal-covariance Gaussian mixture model (.gk / .mc files):
 *
 *   score[t][s] = logsumexp_{j in s} ( log_weight[j] + log_norm[k] - 1/2 sum_d (x_td - mean[k][d])^2 inv_var[k][d] ),
 *   k = kernel[j],  j = state_off[s] .. state_off[s+1] - 1,
 *   log_norm[k] = -1/2 (dim ln 2pi + sum_d ln var[k][d])     (the caller forms it, and 1/var, ln w, in fp64)
 *
 * natural logarithms.  The log-sum-exp takes the state's maximum first; a term whose log weight
 * is -inf (weight 0) contributes nothing; a state without a contributing term, or whose terms
 * are all -inf, scores -inf; a NaN term makes the state NaN (non-finite features propagate).
 * PARITY UNPINNED: phone_probs is not available, the convention is a documented choice.
 * Limits: dim == 39, 1 <= n_kernels <= 256, 1 <= n_states <= 16, at most n_kernels entries a
 * state, kernel indices in range, finite means and normalising constants, finite positive
 * inverse variances, log weights finite or -inf; otherwise SPKD_EINVAL before any device work.
 * d_features: n_frames x 39 floats in device memory (several files may be concatenated);
 * d_scores receives n_frames x n_states floats.  The model arrays are host memory. */
typedef struct {
    int32_t n_kernels, n_states, dim;
    const float *mean;        /* [n_kernels][dim] */
    const float *inv_var;     /* [n_kernels][dim] */
    const float *log_norm;    /* [n_kernels] */
    const int32_t *state_off; /* [n_states + 1], CSR offsets into kernel / log_weight */
    const int32_t *kernel;    /* [state_off[n_states]] kernel index (kernels may be shared) */
    const float *log_weight;  /* [state_off[n_states]] ln of the mixture weight */
} spkd_gmm_params;
spkd_status spkd_gmm_loglik(spkd_ctx *ctx, const float *d_features, int64_t n_frames,
                            const spkd_gmm_params *params, float *d_scores);

/* The decision part of generate_exp.py for a whole batch of files on the device: the scores of
 * n_files files concatenated frame-major, [sum T][n_states] floats as spkd_gmm_loglik leaves them
 * for concatenated features; file f owns the frames [h_frame_off[f], h_frame_off[f+1])
 * (h_frame_off[0] = 0, non-decreasing; a file may have no frames).
 *
 * spkd_vad_shift_batch: shift_dec_bord (generate_exp.py:177-186) per file, with its reshape: the
 * file's block of T * n_states floats is read as (n_states, T), row r = flat [r T, (r + 1) T), and
 * per column, in fp64: exp of every value, row 1 times `shift`, each divided by the sum of the rows
 * in row order, log, rounded to float32 into the same flat position of d_out.  Naive IEEE as the
 * reference: an underflow to 0 gives -inf, 0 / 0 NaN.  d_out may be d_scores (in place).
 * n_states == 1 has no row 1: SPKD_EINVAL.
 *
 * spkd_vad_viterbi_batch: spkd_vad_viterbi for every file in one launch, a group of lanes per file,
 * the same fp64 sums and comparisons in the same order: tokens and scores equal the host
 * function's on the file's slice to the bit.  Out, in pinned memory of the context, valid until
 * its next spkd_vad_viterbi_batch: (*h_tok_off)[n_files + 1], file f's tokens at [tok_off[f],
 * tok_off[f+1]) of *h_tok_frame (first frames, relative to the file) and *h_tok_word;
 * (*h_score)[n_files] the path scores.  A file without frames has no tokens and scores -inf.  The
 * tokens are counted on the device first and then stored at their exact offsets: token memory is
 * 12 bytes per token, not per frame.  Device scratch held by the context: per frame one
 * back-pointer record of 2 bytes (n_words <= 8) or 4 bytes, each file rounded up to SPKD_VAD_TILE
 * frames, the tile in which the kernel fetches scores and stores records.
 * Limits as spkd_vad_viterbi; a bad count, a null pointer, a word state out of range, an
 * h_frame_off that does not start at 0 or decreases: SPKD_EINVAL before any device work.
 * Timers: SPKD_T_VAD_SHIFT, SPKD_T_VAD_VITERBI, SPKD_T_VAD_BACKTRACK (both passes). */
#define SPKD_VAD_TILE 32
spkd_status spkd_vad_shift_batch(spkd_ctx *ctx, const float *d_scores, int64_t n_files,
                                 const int64_t *h_frame_off, int32_t n_states, double shift,
                                 float *d_out);
spkd_status spkd_vad_viterbi_batch(spkd_ctx *ctx, const float *d_scores, int64_t n_files,
                                   const int64_t *h_frame_off, int32_t n_states, int32_t n_words,
                                   const int32_t *h_word_state, const double *h_stay,
                                   const double *h_exit, const double *h_enter,
                                   const int64_t **h_tok_off, const int64_t **h_tok_frame,
                                   const int32_t **h_tok_word, const double **h_score);

/* ---------------------------------------------------------------------------
 * (8) Resegmentation: full-covariance Gaussian speaker models from statistics records and the
 * log-likelihood of every frame of a set of sequences (VAD turns) under the speakers of its file.
 * With spkd_sum_stats in front (speaker records from segment records) and spkd_vad_viterbi_batch
 * behind (sequences = turns, n_states = n_words = n_cols, word_state = identity, stay = exit = 0,
 * enter = -penalty: a speaker loop with a switch penalty; with penalty >= 0 its tie rule, staying
 * beats switching, means a path never re-enters the word it is in) this is the Viterbi
 * resegmentation pass that BIC segmentation + agglomerative clustering systems end with.
 * PARITY: no reference counterpart (the reference stops at clustering); tests/reseg_numpy.py
 * restates both calls in numpy.
 *
 * spkd_gauss_models: one model per record, in fp64.  n = the record's frame count, mu = sum x / n,
 * S = the unbiased covariance (np.cov(rowvar=0), from the moments: (M_ij - (s_i / n) s_j) / (n - 1)),
 * S = L L^T by Cholesky.  A model is SPKD_GAUSS_MODEL = 820 doubles:
 *   [0, 39)    mu
 *   [39, 819)  W = L^-1, packed lower triangle, row-major: W_ij (j <= i) at 39 + i (i + 1) / 2 + j
 *   [819]      c = -1/2 * 39 * ln(2 pi) - sum_i ln L_ii
 * h_ok[i] = 1 when n >= 2 and every pivot is a positive finite number, else 0.  "Positive" is
 * above rounding noise: pivot j must exceed 2^-40 * M_jj / (n - 1), the diagonal entry it started
 * from before the mean was taken out, and a record of fewer than 40 frames, whose covariance has
 * no full rank whatever rounding leaves in its last pivots, is not ok.  So digital silence,
 * constant stretches, fewer than 40 frames and records that are not finite all give 0.  This is
 * no error status: a speaker that cannot be modelled is simply never chosen.  A model that is
 * not ok may hold anything.  One wave per record.
 * n = 0: SPKD_OK without a launch.  A null pointer, buffers that are not 16-byte aligned:
 * SPKD_EINVAL before any device work.  Timer: SPKD_T_GAUSS_MODELS.
 *
 * spkd_gauss_loglik: sequence q covers the absolute frames [h_seq_begin[q], h_seq_end[q]) of
 * d_frames (n_frames x 39 floats); sequences may be empty, need not be contiguous and need not
 * ascend.  It is scored under the models h_seq_model[q] .. + h_seq_n_models[q] - 1 of d_models
 * (n_models models as spkd_gauss_models leaves them, h_model_ok its h_ok).  d_scores is compact:
 * [sum len][n_cols] floats, frame-major, sequence q from row sum_{p < q} len[p] on -- the layout
 * spkd_vad_viterbi_batch reads with h_frame_off set to that running sum.  Column k < n_models(q):
 *   c - 1/2 sum_i y_i^2,   y_i = sum_{j <= i} W_ij (x_j - mu_j)
 * all in fp64 from the float32 frame, rounded once to float32 on the store (as spkd_vad_shift_batch).
 * A model that is not ok gives -inf in its column, and so do the columns n_models(q) .. n_cols - 1.
 * Frames that are not finite propagate NaN.  A workgroup takes a tile of SPKD_GAUSS_TILE frames of
 * one sequence, a lane per frame.
 * Limits: 1 <= n_cols <= 16, 0 <= n_models(q) <= n_cols.  A range outside [0, n_frames] or with
 * end < begin, a model index out of range, a null pointer, d_models not 16-byte aligned:
 * SPKD_EINVAL before any device work, d_scores untouched.  n_seq = 0 or no frame in any sequence:
 * SPKD_OK without a launch.  The index arrays go up in one copy through pinned memory the context
 * owns.  Timer: SPKD_T_GAUSS_LOGLIK. */
#define SPKD_GAUSS_MODEL 820
#define SPKD_GAUSS_TILE 64
spkd_status spkd_gauss_models(spkd_ctx *ctx, const double *d_stats, int64_t n, double *d_models,
                              int32_t *h_ok);
spkd_status spkd_gauss_loglik(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                              const double *d_models, int64_t n_models, const int32_t *h_model_ok,
                              int64_t n_seq, const int64_t *h_seq_begin, const int64_t *h_seq_end,
                              const int32_t *h_seq_model, const int32_t *h_seq_n_models,
                              int32_t n_cols, float *d_scores);

/* spkd_mindur_viterbi_batch: the speaker loop of (8) with a minimum duration.  The shape of
 * spkd_vad_viterbi_batch restricted to that loop: d_scores [sum T][n_cols] floats, sequence q owns
 * the frames [h_frame_off[q], h_frame_off[q+1]) (h_frame_off[0] = 0, non-decreasing; a sequence may
 * be empty), word k is column k (1 <= n_cols <= 16), entering a word costs `penalty` (finite, >= 0),
 * staying and leaving nothing -- and every stretch of a decoded path lasts at least D = min_frames
 * (>= 1) frames.  The one exception is a sequence shorter than D frames, which is a single stretch:
 * every token covers at least D frames or a whole sequence.  A switch penalty cannot promise that:
 * on frames that are correlated in time a short burst beats any penalty that still lets real
 * changes through.  PARITY: no reference counterpart; tests/reseg_mindur_numpy.py restates the
 * recurrence and checks it against a brute-force decoder over the expanded states.
 *
 * The arithmetic, in fp64; the order of the operations is part of the contract:
 *   o_t(k)  the cleaned score, as spkd_vad_viterbi: NaN counts as -inf; a frame whose words are all
 *           -inf counts as 0 for every word.
 *   P_t(k)  the sum of the finite o_u(k), u <= t, added in frame order starting from 0.0;
 *           C_t(k) the number of -inf among them;  P_-1 = C_-1 = 0.
 *   w_t(k)  -inf if C_t(k) - C_{t-D}(k) > 0, otherwise P_t(k) - P_{t-D}(k).
 *   T == 0: no token, score -inf.  T < D: one token (0, k*), k* the lowest k that maximises
 *           (C_{T-1}(k) > 0 ? -inf : P_{T-1}(k)); the score is (-penalty) + that value.
 *   d_t(k)  -inf for t < D - 1;  d_{D-1}(k) = (-penalty) + w_{D-1}(k);  for t >= D, with g and b the
 *           maximum and the lowest arg-max over k of d_{t-D}(k) (for t - D < D - 1: -inf, word 0):
 *             stay = d_{t-1}(k) + o_t(k),  fresh = (g - penalty) + w_t(k),
 *             d_t(k) = stay if stay >= fresh, otherwise fresh with entered_t(k) set.
 *           Staying wins ties.  No NaN can arise: the P are finite.
 *   end     k* the lowest arg-max of d_{T-1}(k); the score is that value.
 *   path    from (T - 1, k*), at (t, j): on t <= D - 1 the token (0, j), and stop; if entered_t(j)
 *           the token (t - D + 1, j), then j = b_{t-D} and t = t - D; otherwise t = t - 1.
 * A sequence whose words all hold a -inf somewhere in every window is what the recurrence makes of
 * it: d stays -inf, and it comes out as the one token (0, 0) with score -inf.  With D = 1 and sums
 * that are exact the tokens and scores are those of spkd_vad_viterbi_batch with stay = exit = 0,
 * enter = -penalty.
 * Out, in pinned memory of the context, valid until its next spkd_mindur_viterbi_batch, laid out as
 * spkd_vad_viterbi_batch's: (*h_tok_off)[n_seq + 1], *h_tok_frame (first frames, relative to the
 * sequence), *h_tok_word, (*h_score)[n_seq].  Device scratch held by the context, per frame, each
 * sequence rounded up to SPKD_MINDUR_TILE frames: the `entered` flags (2 bytes), g (8) and b (4).
 * A bad count, a null pointer, a penalty that is negative or not finite, min_frames < 1, an
 * h_frame_off that does not start at 0 or decreases: SPKD_EINVAL before any device work.
 * Timers: SPKD_T_MINDUR_VITERBI, SPKD_T_MINDUR_BACKTRACK (both passes). */
#define SPKD_MINDUR_TILE 32
spkd_status spkd_mindur_viterbi_batch(spkd_ctx *ctx, const float *d_scores, int64_t n_seq,
                                      const int64_t *h_frame_off, int32_t n_cols, double penalty,
                                      int32_t min_frames,
                                      const int64_t **h_tok_off, const int64_t **h_tok_frame,
                                      const int32_t **h_tok_word, const double **h_score);

/* spkd_fb_posterior_batch: how sure the speaker loop of (8) is of what it decodes.  A forward-backward
 * pass over the scores the decoders search, with their loop (staying costs nothing, a switch `penalty`):
 * the posterior probability of every speaker at every frame of every sequence, per decoded token the
 * mean posterior of its word over its frames (the confidence of the row it becomes), and the
 * log-evidence of each sequence.  The decoded path of spkd_vad_viterbi_batch is the mode of this
 * distribution; the confidence says how much of the mass sits near it.  Under a minimum duration
 * (spkd_mindur_viterbi_batch) the posterior is still that of the plain switch-penalty loop.  PARITY: no
 * reference counterpart; tests/reseg_fb_numpy.py restates the recursion and checks it against an
 * enumeration of all paths.
 *
 * In: d_scores, h_frame_off, n_cols (1 .. 16) and penalty (finite, >= 0) as spkd_mindur_viterbi_batch
 * takes them.  scale: finite, > 0, scale * penalty <= 600 -- an acoustic scale on the whole path
 * log-weight (the decoded path is the mode for every scale).  h_seq_n_cols[n_seq]: sequence q uses the
 * columns 0 .. n(q) - 1, 1 <= n(q) <= n_cols; NULL: n_cols for every sequence.  The tokens as the
 * decoders hand them back: h_tok_off[n_seq + 1], h_tok_frame (first frames, relative to the sequence),
 * h_tok_word; all three NULL: no confidences.  d_post: NULL or [sum T][n_cols] floats.  h_conf[n_tok]
 * (with tokens) and h_logz[n_seq]: doubles, the caller's.
 *
 * The values, all in fp64; n = n(q), k < n.  This fixes values, not the order of the operations:
 *   o_t(k)   the cleaned score, as spkd_vad_viterbi: NaN counts as -inf; a frame whose n words are all
 *            -inf counts as 0 for every word.  m_t = max_k o_t(k), b_t(k) = exp(scale (o_t(k) - m_t)).
 *            The columns >= n take no part; their posterior is 0.
 *   q, r     q = exp(-scale penalty), r = 1 - q.
 *   forward  u_0(k) = b_0(k), u_t(k) = b_t(k) (r a_{t-1}(k) + q), s_t = sum_k u_t(k),
 *            a_t(k) = u_t(k) / s_t, logz = -scale penalty + sum_t (scale m_t + ln s_t).  At scale 1 logz
 *            is on the scale of the decoders' path scores and never below the plain decoder's.
 *   backward beta_{T-1}(k) = 1, h(k) = b_{t+1}(k) beta_{t+1}(k), H = sum_k h(k), w(k) = r h(k) + q H,
 *            beta_t(k) = w(k) / sum_k w(k).
 *   gamma    gamma_t(k) = a_t(k) beta_t(k) / sum_j a_t(j) beta_t(j).
 * Every divisor is positive: s_t >= q, beta >= q / 16, the last sum >= q / 256 -- hence the cap on
 * scale * penalty.  A b that underflows to 0 is a posterior of 0.
 * Out: d_post receives gamma rounded once to float32, 0 in the columns >= n(q).  h_conf[i], for the token
 * (f_i, word) of sequence q, is the mean of gamma_t(word) over [f_i, f_{i+1}); a sequence's last token
 * runs to T.  T == 0: logz = -inf.  A +inf score makes that sequence's outputs NaN and nothing else.
 * One launch: a group of lanes per sequence runs forward, keeping only the forward vector that enters
 * each tile of SPKD_FB_TILE frames (fp64: device scratch of 8 G bytes a tile, G the power of two >=
 * n_cols), then backward tile by tile, rebuilding the tile's forward vectors from the stored one.
 * A bad count or a null required pointer; an h_frame_off that does not start at 0 or decreases; an n(q)
 * outside 1 .. n_cols; a bad penalty or scale, scale * penalty > 600; a token table given in part; an
 * h_tok_off that does not start at 0 or decreases; a sequence with frames whose tokens do not start at
 * frame 0, do not ascend strictly or reach T; tokens on a sequence without frames; a word outside
 * 0 .. n_cols - 1: SPKD_EINVAL before any device work.  n_seq = 0: SPKD_OK; no frames anywhere: every
 * logz -inf and SPKD_OK; both without a launch.  The index and token arrays go up in one copy through
 * pinned memory the context owns.  Timer: SPKD_T_FB_POSTERIOR. */
#define SPKD_FB_TILE 32
spkd_status spkd_fb_posterior_batch(spkd_ctx *ctx, const float *d_scores, int64_t n_seq,
                                    const int64_t *h_frame_off, int32_t n_cols, double penalty,
                                    double scale, const int32_t *h_seq_n_cols,
                                    const int64_t *h_tok_off, const int64_t *h_tok_frame,
                                    const int32_t *h_tok_word, float *d_post, double *h_conf,
                                    double *h_logz);

/* spkd_post_stats: statistics records from frames weighted by their posteriors -- what turns the
 * posteriors of spkd_fb_posterior_batch into speakers again (Baum-Welch retraining: every speaker of a
 * file is trained on all frames of the file's turns, each weighted by the speaker's posterior there,
 * instead of on the frames a decoded path gave it wholly).  PARITY: no reference counterpart;
 * tests/reseg_soft_numpy.py restates it.
 *
 * In: the sequences, h_seq_model, h_seq_n_models and n_cols exactly as spkd_gauss_loglik takes them.
 * d_post: the compact [sum len][n_cols] float32 array in that call's score layout, which is the layout
 * spkd_fb_posterior_batch writes its d_post in.  Out: d_stats receives n_models records in the layout
 * of spkd_set_stats: the packed upper triangle of the 40 x 40 augmented moment matrix, 820 doubles,
 * the count at pk(39, 39), the last entry.
 *
 * The values, all in fp64.  For model m take every sequence q with
 * h_seq_model[q] <= m < h_seq_model[q] + h_seq_n_models[q]; for every frame t of q let
 * w = (double) d_post[row(q, t)][m - h_seq_model[q]]; the record adds w * x~ x~^T, x~ = (x, 1), x the
 * float32 frame converted once.
 *   A weight that is exactly 0 contributes nothing, whatever the frame holds: a frame that is not
 *   finite under weight 0 leaves the record finite (the kernel passes such frames over).
 *   Any other weight or frame that is not finite propagates; spkd_gauss_models then answers ok = 0
 *   for that record.
 *   Every record 0 .. n_models - 1 is written; a model no sequence covers gets zeros.
 *   The model ranges of two sequences with models are either identical (the turns of one file) or
 *   disjoint (different files); anything else is SPKD_EINVAL.
 * This fixes values, not the order of the operations.  There are no float atomics: the bits of a
 * record depend neither on the run nor on the grid nor on the other files of the call -- they are a
 * function of the model's own sequences in the order the call lists them.
 * Two launches: one workgroup per (chunk of SPKD_POST_CHUNK frames of a sequence, column) sums its
 * frames, 820 FMAs a frame and column; then every model adds its workgroups' partial records in
 * (sequence, chunk) order.  Device scratch held by the context: 6 560 bytes a workgroup.
 * Limits and refusals are those of spkd_gauss_loglik: 1 <= n_cols <= 16, 0 <= n_models(q) <= n_cols;
 * a range outside [0, n_frames] or with end < begin, a model index outside [0, n_models], a null
 * pointer, a d_stats that is not 16-byte aligned: SPKD_EINVAL before any device work, d_stats
 * untouched.  n_models = 0: SPKD_OK without a launch.  The index arrays go up in one copy through
 * pinned memory the context owns.  Timer: SPKD_T_POST_STATS (all launches of the call). */
#define SPKD_POST_CHUNK 1024
spkd_status spkd_post_stats(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                            const float *d_post, int64_t n_seq,
                            const int64_t *h_seq_begin, const int64_t *h_seq_end,
                            const int32_t *h_seq_model, const int32_t *h_seq_n_models,
                            int32_t n_cols, int64_t n_models, double *d_stats);

/* ---------------------------------------------------------------------------
 * (9) Resegmentation with mixture models: a diagonal-covariance Gaussian mixture per speaker,
 * trained by EM on the device from the speaker's own frames, and the log-likelihood of every frame
 * of a set of sequences under the mixtures of its file's speakers.  These two calls stand where
 * spkd_sum_stats + spkd_gauss_models and spkd_gauss_loglik stand in (8); the decoder behind them is
 * the same spkd_vad_viterbi_batch call.  One full-covariance Gaussian suits a comparison of whole
 * segments; a frame-level decoder on speech, whose frames fall into several phonetic modes, is
 * better served by a small mixture.
 * PARITY: no reference counterpart; tests/reseg_gmm_numpy.py restates both calls in numpy.
 *
 * A speaker model is n_comp = K components of SPKD_GMM_COMP = 80 doubles, speaker s at
 * d_gmm + s * K * 80:
 *   [0]        ln w
 *   [1, 40)    mean
 *   [40, 79)   1 / var
 *   [79]       log_norm = -1/2 (39 ln 2pi + sum_d ln var_d)
 *
 * spkd_gmm_train: speaker s owns the absolute frame ranges [h_range_begin[r], h_range_end[r]) for r
 * in h_set_off[s] .. h_set_off[s + 1], in that order; its frames are numbered 0 .. N - 1 in that
 * order.  All arithmetic is fp64 on the float32 frames.
 *   V_d, the ML (biased) variance of all N frames, sets the floor var_floor * V_d of every variance.
 *   Initial model (from_model = 0), "segmental": component k takes the frames with the ordinals
 *     [floor(k N / K), floor((k + 1) N / K)): w = count / N, their mean and ML variance, floored.
 *   from_model != 0: the start is what d_gmm holds.
 *   An iteration: with l_k = ln w_k + log_norm_k - 1/2 sum_d (x_d - mean_kd)^2 / var_kd,
 *     m = max_k l_k and g_k = exp(l_k - m) / sum_j exp(l_j - m) per frame (a component whose ln w
 *     is -inf takes no part), G_k = sum g_k, A_kd = sum g_k x_d, B_kd = sum g_k x_d^2 and
 *     L = sum (m + ln sum_j exp(l_j - m)) over the frames; h_loglik[s * n_iter + i] = L of the model
 *     that entered iteration i.  Then w_k = G_k / N (ln w = -inf for G_k = 0) and, when G_k >= 2,
 *     mean = A / G, var = max(B / G - mean^2, var_floor * V_d); otherwise the component keeps its
 *     mean and variance.
 *   h_ok[s] = 0, without an error status, when N < 40 K, when a V_d is not a finite number > 0
 *   (constant frames, frames that are not finite), when an accumulator or L of any step is not
 *   finite, or when a model value written is not finite (a variance of 0 under var_floor = 0): the
 *   rule of spkd_gauss_models -- a speaker that cannot be modelled is never chosen.  Its model may
 *   hold anything.
 *   n_iter = 0 is the initial model alone.  The whole loop is enqueued on the context's stream
 *   inside the one call, with no host trip between iterations; h_ok and h_loglik come back once,
 *   through pinned memory the context owns, as the index arrays go up in one copy.
 *   Determinism: a speaker's ordinals are cut into tiles of SPKD_GMM_TILE = 64 and chunks of
 *   SPKD_GMM_CHUNK_TILES = 16 tiles; every sum runs in ordinal order inside a chunk and in chunk
 *   order across them, without atomics.  The bits of a speaker's model depend neither on the run
 *   nor on the grid nor on the other speakers of the call, and n_iter = n in one call equals n
 *   calls of n_iter = 1 with from_model = 1.
 *   SPKD_EINVAL before any device work, outputs untouched: a null pointer (h_loglik may be NULL
 *   when n_iter = 0), K outside [1, SPKD_GMM_MAX_COMP = 8], n_iter < 0, var_floor not finite or < 0,
 *   h_set_off not starting at 0, a set without a range, a range outside [0, n_frames] or with
 *   end < begin, d_gmm not 16-byte aligned.  n_speakers = 0: SPKD_OK without a launch.
 *   Timer: SPKD_T_GMM_TRAIN (all launches of the call).
 *   Accuracy domain (against this section stated at 50 digits with centred variances,
 *   tests/test_mixture_exact.py; measure |a - b| / max(1, |a|, |b|); table in DESIGN.md section 5,
 *   "Mixture speaker models"): var = B / G - mean^2 is a difference of raw moments and loses
 *   mean^2 / var, so the error of 1 / var grows with the square of a component mean's distance from
 *   the origin in sigma: 2e-14, 2e-13 and 8e-12 at 1, 8 and 64 sigma.  A trained model, its L, the
 *   scores and spkd_ubm_stats' records are good to 1e-9 up to the 64 sigma that are tested; that law
 *   continued reaches 1e-9 near 700 sigma and 1e-5 near 70 000 sigma (not tested).  A frame as large
 *   as 3e38 is finite and leaves h_ok at 1, but every other value of its dimension is below half an
 *   ulp beside it: such a frame decides nothing.  A caller whose features are not centred subtracts
 *   one constant vector per file first, as for spkd_set_stats.
 *
 * spkd_gmm_loglik_seq: spkd_gauss_loglik with mixtures: column k < n_models(q) of a frame is
 *   m + ln sum_j exp(l_j - m) under the sequence's k-th speaker (n_models models of n_comp components
 *   in d_gmm, h_model_ok spkd_gmm_train's h_ok), in fp64, rounded once to float32 on the store.  A
 *   model that is not ok and the columns past the sequence's models give -inf; frames that are not
 *   finite propagate NaN.  Compact scores, limits (1 <= n_cols <= 16), refusals (and n_comp outside
 *   [1, 8]), the one upload of the index arrays and the tile (SPKD_GMM_TILE) are spkd_gauss_loglik's.
 *   Timer: SPKD_T_GMM_SEQ_LOGLIK. */
#define SPKD_GMM_COMP 80
#define SPKD_GMM_MAX_COMP 8
#define SPKD_GMM_TILE 64
#define SPKD_GMM_CHUNK_TILES 16
spkd_status spkd_gmm_train(spkd_ctx *ctx, const float *d_frames, int64_t n_frames, int64_t n_speakers,
                           const int64_t *h_set_off, const int64_t *h_range_begin,
                           const int64_t *h_range_end, int32_t n_comp, int32_t n_iter,
                           int32_t from_model, double var_floor, double *d_gmm, int32_t *h_ok,
                           double *h_loglik);
spkd_status spkd_gmm_loglik_seq(spkd_ctx *ctx, const float *d_frames, int64_t n_frames,
                                const double *d_gmm, int32_t n_comp, int64_t n_models,
                                const int32_t *h_model_ok, int64_t n_seq, const int64_t *h_seq_begin,
                                const int64_t *h_seq_end, const int32_t *h_seq_model,
                                const int32_t *h_seq_n_models, int32_t n_cols, float *d_scores);

/* ---------------------------------------------------------------------------
 * (10) Linking speakers across files by cross-likelihood ratio: every speaker's zeroth- and
 * first-order statistics under one universal background model (UBM), and agglomerative clustering of
 * those records under MAP-adapted means.  One full-covariance Gaussian (spkd_sum_stats + spkd_ahc
 * with BIC) suits a segment; a whole speaker's frames fall into several modes whose shares differ
 * from recording to recording, and over 10^3 .. 10^5 frames no BIC penalty bridges the two Gaussians
 * that gives.  The records add under a merge, so the frames are read once.
 * PARITY: no reference counterpart; tests/link_clr_numpy.py restates both calls in numpy.
 *
 * The UBM is ONE model of n_comp = C components in spkd_gmm_train's layout (SPKD_GMM_COMP doubles a
 * component), e.g. spkd_gmm_train's model of one speaker that owns the ranges of all speakers.  A
 * speaker record is C components of SPKD_BW_COMP = 40 doubles, speaker s at d_bw + s * C * 40:
 *   [0]        n_c = sum g_c(x)
 *   [1, 40)    f_c = sum g_c(x) x
 * over the speaker's frames, g_c exactly the g_k of spkd_gmm_train's iteration under the UBM (a
 * component whose ln w is -inf takes no part: its n and f are 0).  All arithmetic is fp64 on the
 * float32 frames.
 *
 * spkd_ubm_stats: the speakers and their frames are given as to spkd_gmm_train (h_set_off,
 *   h_range_begin, h_range_end; a range may be empty).  Determinism is spkd_gmm_train's: tiles of
 *   SPKD_GMM_TILE ordinals, chunks of SPKD_GMM_CHUNK_TILES tiles, ordinal order inside a chunk and
 *   chunk order across chunks, no atomics; the bits of a record depend neither on the run nor on the
 *   grid nor on the other speakers of the call.  Every frame is read once (156 bytes); the index
 *   arrays go up in one copy through pinned memory the context owns, h_ok comes back once.
 *   h_ok[s] = 0, without an error status, when the speaker has no frame or when a sum is not finite.
 *   SPKD_EINVAL before any device work, outputs untouched: spkd_gmm_train's rules for the pointers,
 *   the sets and the ranges, C outside [1, SPKD_GMM_MAX_COMP], d_ubm or d_bw not 16-byte aligned.
 *   n_speakers = 0: SPKD_OK without a launch.  Timer: SPKD_T_UBM_STATS (both launches).
 *
 * spkd_clr_link: the whole agglomerative chain over n records in one call, no host trip per merge.
 *   With the UBM's means mu and variances, the relevance r and N = sum_c n_c (component order):
 *     m_c = (f_c + r mu_c) / (n_c + r)                                   (MAP, means only)
 *     H(a|b) = (1 / N_a) sum_c sum_d [(m^b_cd - mu_cd) f^a_cd - 1/2 n^a_c ((m^b_cd)^2 - mu_cd^2)] / var_cd
 *     CLR(a, b) = H(a|b) + H(b|a)                                        (higher: more alike)
 *   H(a|b) is the log-likelihood ratio per frame of a's frames under b's adapted model against the
 *   UBM at the UBM's alignment.  A step: over the clusters whose h_ok is set, the pair a < b of the
 *   highest CLR, the first in row-major order on a tie.  It is merged when CLR > threshold, or when
 *   max_spk > 0 and more than max_spk clusters are in the list (those whose h_ok is 0 included);
 *   otherwise, and when fewer than two ok clusters are left, the chain stops.  A merge is
 *   record[a] += record[b] and speakers.pop(b): later indices shift down, the convention of spkd_ahc's
 *   log, replayable by spkd_labels_from_merges.  Only row and column a are computed again.  A speaker
 *   whose h_ok is 0 is never chosen and keeps its own label (the rule of spkd_gauss_models).
 *   h_merge_a / h_merge_b / h_merge_d take up to n - 1 entries; h_stat_max / h_stat_min are the
 *   extremes of the initial matrix (NaN when it has no pair).  d_bw is not modified.
 *   A CLR among ok speakers that is not finite: SPKD_ENONFINITE, with the log so far.
 *   Accuracy domain: the terms (m - mu) f and 1/2 n (m^2 - mu^2) cancel, so the ratio loses digits with
 *   the square of the UBM means' distance from the origin in sigma.  Measured against exact arithmetic
 *   (tests/exact_clr.py; ratios of a few units, C = 8): 2e-15 at 0 sigma, 9e-15 at 8 sigma (one digit),
 *   4e-13 at 64 sigma (three digits), 2e-10 at 1 024 sigma (five to six digits).  Cepstral-mean-normalised
 *   features, the default, keep the UBM's means within a few sigma of 0, far inside.  A record whose N
 *   is 0 (all zeros) with h_ok set makes the ratio 0 / 0: SPKD_ENONFINITE.
 *   Limits: n <= SPKD_CLR_MAX_N = 4096 (the chain is one workgroup whose per-row state waits in LDS;
 *   the matrix is n^2 doubles of device scratch).  SPKD_EINVAL before any device work, outputs
 *   untouched: a null pointer, n above the limit, C outside [1, SPKD_GMM_MAX_COMP], r not finite or
 *   <= 0, threshold NaN, max_spk < 0, d_bw or d_ubm not 16-byte aligned.  n = 0: SPKD_OK without a
 *   launch; n = 1: no merge.  Timer: SPKD_T_CLR_LINK (all launches of the call). */
#define SPKD_BW_COMP 40
#define SPKD_CLR_MAX_N 4096
spkd_status spkd_ubm_stats(spkd_ctx *ctx, const float *d_frames, int64_t n_frames, const double *d_ubm,
                           int32_t n_comp, int64_t n_speakers, const int64_t *h_set_off,
                           const int64_t *h_range_begin, const int64_t *h_range_end, double *d_bw,
                           int32_t *h_ok);
spkd_status spkd_clr_link(spkd_ctx *ctx, const double *d_bw, int64_t n, const int32_t *h_ok,
                          const double *d_ubm, int32_t n_comp, double relevance, double threshold,
                          int32_t max_spk, int32_t *h_merge_a, int32_t *h_merge_b, double *h_merge_d,
                          int32_t *h_n_merges, double *h_stat_max, double *h_stat_min);

/* ---------------------------------------------------------------------------
 * (10b) Feature warping (Pelecanos & Sridharan 2001) ahead of section 10: over a sliding window of a
 * file's speech every coefficient is replaced by the standard-normal quantile of its rank in the
 * window.  The result does not change under any increasing distortion of a dimension -- the gain and
 * offset by which two microphones differ at the least, which the background model, the adapted means
 * and the ratio of section 10 all take for a speaker difference -- and it is N(0, 1)-like, the regime
 * section 10's accuracy note calls far inside.
 * PARITY: no reference counterpart; tests/warp_numpy.py restates the rule frame by frame.
 *
 * The rule.
 *   Sets and runs.  A set is one file's speech: the frame ranges [begin, end) h_set_off[s] ..
 *     h_set_off[s + 1] of h_range_begin / h_range_end, ascending and disjoint over the whole list (a
 *     range may be empty, two may touch, a set may have none).  Concatenated they are the set's
 *     compacted axis j = 0 .. L - 1.
 *   Window.  With n = min(window, L), frame j sees the compacted frames [lo, lo + n),
 *     lo = clamp(j - n / 2, 0, L - n) (integer division).  The window slides inside the set: it never
 *     crosses into another set and never sees a frame that lies in no range.
 *   Counts.  Per dimension d, with v the frame's value: lt is the number of window values < v, eq the
 *     number == v, as float32 compares.  The frame counts itself, so eq >= 1 unless v is a NaN, and
 *     -0.0 == 0.0.
 *   Output.  out = table_n[2 lt + eq - 1] with table_n[k - 1] = float32(Phi^-1(k / (2 n))) for
 *     k = 1 .. 2 n - 1.  Without ties that is Pelecanos' (rank - 1/2) / n; with ties it is the
 *     mid-rank, symmetric and independent of order.
 *   NaN and infinities.  A NaN value gives the quiet NaN 0x7fc00000 and counts in nobody's lt or eq; n
 *     stays what it is.  +-inf compare as usual.
 *   Frames outside the ranges.  A frame of d_out that lies in no range is not written.
 *
 * spkd_feature_warp: d_frames and d_out hold n_frames frames of 39 floats.  The caller supplies the
 *   quantile tables: set s, when it has a frame, reads the 2 n - 1 floats at h_table + h_table_off[s]
 *   (sets of the same n share a table; the entry of a set without a frame is not looked at).  The
 *   library computes no inverse CDF: device and restatement read the same bits.
 *   One workgroup per tile of SPKD_WARP_TILE compacted frames of one set; the tile and its halo go
 *   through the run table into LDS once, dimension-major, and the counts run from there.  Integer
 *   counts and one look-up, no atomics: the bits depend neither on the run nor on the tiling nor on
 *   the other sets of the call.  The tables go up in one copy through pinned memory the context owns.
 *   SPKD_EINVAL before any device work, outputs untouched: a null pointer, n_frames or n_sets < 0,
 *   window outside [1, SPKD_WARP_MAX_WINDOW = 512], offsets that do not start at 0 or that decrease, a
 *   range outside [0, n_frames] or with end < begin, ranges that are not ascending and disjoint over
 *   the whole list, a set of more than 2^31 - 1 frames, a table slice that does not lie in
 *   [0, table_len], d_frames or d_out not 16-byte aligned, d_out overlapping d_frames (in place cannot
 *   work: neighbours are read).  No frame in any range: SPKD_OK without a launch.
 *   Timer: SPKD_T_FEATURE_WARP. */
#define SPKD_WARP_MAX_WINDOW 512
#define SPKD_WARP_TILE 384
spkd_status spkd_feature_warp(spkd_ctx *ctx, const float *d_frames, int64_t n_frames, int64_t n_sets,
                              const int64_t *h_set_off, const int64_t *h_range_begin,
                              const int64_t *h_range_end, int32_t window, const float *h_table,
                              int64_t table_len, const int64_t *h_table_off, float *d_out);

/* ---------------------------------------------------------------------------
 * (11) A gallery of enrolled speakers: the records of section 10, kept from one batch to the next,
 * and the identification of a batch's speakers against them.  The global labels of spkd_clr_link are
 * positions in the list of ONE call; an identity of a gallery means the same person in every call.
 * The records of a gallery and of its probes are comparable only under the UBM they were collected
 * under (spkd_ubm_stats takes the model as an argument: the owner of the gallery keeps it).
 * PARITY: no reference counterpart (spk-clustering.py:289 is a TODO for more than one wav);
 * tests/gallery_numpy.py restates both calls in numpy.
 *
 * spkd_clr_identify: n_probe records at d_probe_bw against n_gallery records at d_gallery_bw, both in
 *   the layout of section 10 under the UBM at d_ubm.
 *     score[s][g] = CLR(probe s, identity g)          (section 10; the bits are those spkd_clr_link's
 *                                                      initial matrix holds for the same two records)
 *   for every probe and identity whose ok flag is set, NaN elsewhere.  All arithmetic is fp64, no
 *   atomics on values: the bits depend neither on the run nor on the tiling.  T and N of the gallery
 *   are derived once per call.
 *   The probes come in n_groups groups, group k the probes h_group_off[k] .. h_group_off[k + 1] (a
 *   group may be empty): the probes of a group must receive distinct identities -- the speakers of one
 *   file, the clusters of one batch.  exclusive = 1: a greedy chain per group.  Among the group's
 *   undecided ok probes and the ok identities not yet taken IN THIS GROUP, the pair of the highest
 *   score, the first in row-major order on a tie (spkd_clr_link's rule); while that score is above
 *   `threshold` the pair is assigned, the probe and the identity are closed, and the chain goes on;
 *   otherwise it stops and the probes left over are unknown.  exclusive = 0: every ok probe takes the
 *   identity of its highest score (the lowest index on a tie) when that is above the threshold; no
 *   identity is closed.
 *   h_ident[s]: the identity, or -1 (unknown).  h_score[s]: the assigned pair's score; of an unknown
 *   probe its highest score over all ok identities.  h_second[s]: the probe's highest score over the ok
 *   identities other than the reported one -- of an unknown probe: other than the first that reaches
 *   h_score -- or NaN when there is none.  Neither depends on the order of the chain beyond the
 *   identity itself.  A probe that is not ok: ident -1, score and second NaN.  An identity that is not
 *   ok is never chosen.  d_scores: NULL, or n_probe * n_gallery doubles that receive the matrix (row s
 *   at d_scores + s * n_gallery).
 *   A score between an ok probe and an ok identity that is not finite: SPKD_ENONFINITE, every ident -1,
 *   score and second NaN.
 *   Limits: n_probe <= SPKD_CLR_MAX_N and n_groups <= SPKD_CLR_MAX_N (a group is one workgroup whose
 *   per-row state waits in LDS), n_gallery <= SPKD_GALLERY_MAX_N = 16384 (one bit a column there).  The
 *   matrix is n_probe * n_gallery doubles of device scratch unless d_scores is given, at most 512 MB;
 *   the derived records take n_gallery * C * 40 doubles more.
 *   SPKD_EINVAL before any device work, outputs untouched: a null pointer other than d_scores (the
 *   gallery's two may be null when n_gallery = 0), a negative count or one above its limit, group
 *   offsets that do not start at 0, go back or do not end at n_probe, C outside
 *   [1, SPKD_GMM_MAX_COMP], r not finite or <= 0, threshold NaN, exclusive other than 0 or 1, a device
 *   pointer that is not 16-byte aligned.  n_probe = 0: SPKD_OK without a launch.  n_gallery = 0:
 *   SPKD_OK without a launch, every probe unknown, score and second NaN.
 *   Timers: SPKD_T_IDENT_SCORES (the derived records and the matrix), SPKD_T_IDENT_ASSIGN.
 *
 * spkd_bw_accumulate: ordered sums of records, what a merge of section 10 does to a record:
 *     dst[h_dst[k]] = (h_keep[k] ? dst[h_dst[k]] : 0) + src[m_0] + src[m_1] + ...
 *   over the members m_i = h_member[h_set_off[k] ..  h_set_off[k + 1]) of set k, in that order, by plain
 *   fp64 additions, one element a lane: the bits are those of the sum written down in that order.  A
 *   set may be empty.  The records of d_src_bw (n_src of them) and d_dst_bw (n_dst) must not overlap.
 *   SPKD_EINVAL before any device work, d_dst_bw untouched: a null pointer, a negative count, more sets
 *   than slots, offsets that do not start at 0 or go back, a member outside [0, n_src), a slot outside
 *   [0, n_dst) or named twice, C outside [1, SPKD_GMM_MAX_COMP], a buffer that is not 16-byte aligned.
 *   n_sets = 0: SPKD_OK without a launch.  Timer: SPKD_T_BW_ACCUMULATE. */
#define SPKD_GALLERY_MAX_N 16384
spkd_status spkd_clr_identify(spkd_ctx *ctx, const double *d_probe_bw, int64_t n_probe,
                              const int32_t *h_probe_ok, int64_t n_groups, const int64_t *h_group_off,
                              const double *d_gallery_bw, int64_t n_gallery, const int32_t *h_gallery_ok,
                              const double *d_ubm, int32_t n_comp, double relevance, double threshold,
                              int32_t exclusive, int32_t *h_ident, double *h_score, double *h_second,
                              double *d_scores);
spkd_status spkd_bw_accumulate(spkd_ctx *ctx, const double *d_src_bw, int64_t n_src, int32_t n_comp,
                               int64_t n_sets, const int64_t *h_set_off, const int32_t *h_member,
                               const int32_t *h_dst, const int32_t *h_keep, double *d_dst_bw,
                               int64_t n_dst);

/* ---------------------------------------------------------------------------
 * (5) Host-side helpers of the boundary (no GPU work).
 *
 * spkd_py2_roundtrip: v[i] <- float(str(v[i])) with Python-2 str() = "%.12g":
 * the value the next stage reads back from a recipe time this stage writes
 * (spk-change-detection.py:59-60 -> spk-clustering.py:16-23).
 *
 * spkd_labels_from_merges: replays a merge log of spkd_ahc
 * (speakers[a].extend(speakers[b]); speakers.pop(b), spk-clustering.py:216-217)
 * and returns for each of the n initial records its final 1-based cluster index.
 */
void spkd_py2_roundtrip(double *h_values, int64_t n);
spkd_status spkd_labels_from_merges(int64_t n, int64_t n_merges, const int32_t *h_a,
                                    const int32_t *h_b, int32_t *h_labels);
/* the same for n_problems merge logs laid out like spkd_ahc's outputs (problem p:
 * records h_seg_off[p] .. h_seg_off[p+1], merges at h_seg_off[p] + m) */
spkd_status spkd_labels_from_merges_batch(int64_t n_problems, const int64_t *h_seg_off,
                                          const int32_t *h_n_merges, const int32_t *h_a,
                                          const int32_t *h_b, int32_t *h_labels);

/* Host-side: detections per turn of an spkd_gw result -- out[t] = number of non-zero flags
 * among h_flags[h_off[t] .. h_off[t] + h_n[t]) (the h_win_det entries of turn t's h_n_win[t]
 * windows; what lies behind them in a reused buffer is not looked at). */
spkd_status spkd_count_flags(const int32_t *h_flags, const int64_t *h_off, const int32_t *h_n,
                             int64_t n_groups, int32_t *h_out);

/* Host-side: the recipe lines of an spkd_gw result in recipe order -- per turn its h_n_det[t]
 * detections (detection j: [start, start + maxi) of the turn, event slot h_off[t] + j), then
 * the tail line [final start, turn end) -- as the change-detection script writes them
 * (spk-change-detection.py:374-392): h_times[2 i], h_times[2 i + 1] = start / end in seconds,
 * start_s + frames / rate in the reference's operation order, passed through
 * spkd_py2_roundtrip when text_contract is non-zero.  Optional (NULL to skip): the absolute
 * frame range [h_frame_b[i], h_frame_e[i]) whose statistics the fused detector left for the
 * line, the event slot h_index[i] of that record, the turn h_line_turn[i] of the line.
 * n_lines must be n_turns + the sum of h_n_det. */
spkd_status spkd_gw_lines(int64_t n_turns, const int64_t *h_off, const int32_t *h_n_det,
                          const double *h_det_start, const double *h_det_maxi,
                          const double *h_final_start, const double *h_turn_start_s,
                          const double *h_turn_end_s, const int64_t *h_turn_begin,
                          const int64_t *h_turn_end, double rate, int text_contract,
                          int64_t n_lines, double *h_times, int64_t *h_frame_b,
                          int64_t *h_frame_e, int64_t *h_index, int32_t *h_line_turn);

/* Host-side: the speech / non-speech decoding of generate_exp.py (its AaltoASR token pass,
 * generate_exp.py:189-239) for a loop of one-state words, as an exact Viterbi in fp64.
 * Word j emits state h_word_state[j] of h_scores (n_frames x n_states floats, frame-major, the
 * .lna layout); a NaN score counts as -inf, a frame whose words all score -inf counts as 0 for
 * every word.  With the per-word constants the caller forms (stay = ts ln a_jj,
 * exit = ts ln a_j,exit, enter = lm ln(10) log10 P(j) - ins):
 *
 *   d_0(j) = enter_j + obs_0(j)
 *   d_t(j) = max( d_{t-1}(j) + stay_j , max_i(d_{t-1}(i) + exit_i) + enter_j ) + obs_t(j)
 *
 * i over every word, j included.  Ties: staying beats switching, the lowest i, and at the end
 * the lowest j, win.  Out: the tokens of the best path -- the first frame and the word of every
 * word it enters, in order (at most n_frames: the caller's arrays hold n_frames entries) -- and
 * its score max_j d_{T-1}(j) (-inf for no frames).  Limits: 1 <= n_states, n_words <= 16. */
spkd_status spkd_vad_viterbi(int64_t n_frames, int32_t n_states, const float *h_scores,
                             int32_t n_words, const int32_t *h_word_state, const double *h_stay,
                             const double *h_exit, const double *h_enter, int64_t *h_tok_frame,
                             int32_t *h_tok_word, int64_t *h_n_tokens, double *h_score);

#ifdef __cplusplus
}
#endif
#endif /* SPKD_H */
