// Neighbour merge (merge_rec, spk-change-detection.py:136-177, driven by :375-394) for a whole
// batch: a problem is one file's recipe lines in order, line k the frame range [b_k, e_k).
//
//   k_merge_flags       : per record, whether a covariance of it can be formed at all
//   k_merge_ahead       : per adjacent pair of lines AS THE RECIPE NAMES THEM, the determinant a
//                         step needs when its left side is the unmerged line (all CUs)
//   k_merge_chain_batch : the decision chain, one wave per problem
//
// The script compares `prev`, the run merged so far, with the next line.  prev's frames are
// features[start_first * rate : end_last * rate], so the run spans the gaps inside it; the pooled
// array of a step is np.concatenate((arr1, arr2)), so the gap in front of the next line is not in
// the union.  On records (R_k: line k, G_k: the gap [e_k, b_{k+1}), absent when empty):
//   left side L     = R_first at the start of a run; after merging line k + 1: L <- (L + G_k) + R_{k+1}
//   union of a step = L + R_{k+1} (formed by quad_pair_det, never stored)
//   no merge        : L <- R_{k+1}
// The additive form needs lines that neither overlap nor go backwards; the host refuses others.
//
// A step's elimination is quad_pair_det(kind, L staged in LDS, .., the next line's records): the
// ahead pass calls it with L = R_k for every k, the chain with the running L behind a merge --
// the same device function with the same operands in the same order, so a step's distance does
// not depend on which of the two computed it.  KL2 needs no elimination per pair: its ahead pass
// is k_cluster_prep_batch's vectors, and the chain recomputes L's vectors behind a merge.
#pragma once
#include "spkd_cluster.hpp"

namespace spkd {

constexpr int MRG_AHEAD_WAVES = 4;           // pairs per workgroup of the ahead pass (15 KB of LDS each)

// flags[r] = 1 when record r holds an inf or a NaN, or -- the n_lines line records only -- fewer
// than two frames: np.cov of such a set has infs or NaNs, and the reference's det raises.  (A gap
// of one frame is fine: it only ever enters a sum.)  One wave per record.
__global__ __launch_bounds__(WAVE) void k_merge_flags(const double* __restrict__ pk, int64_t n_rec, int64_t n_lines,
                                                      int32_t* __restrict__ flags) {
    const int64_t r = blockIdx.x;
    if (r >= n_rec) return;
    const double* g = pk + r * REC;
    bool bad = false;
    for (int e = lane_id(); e < REC; e += WAVE) bad |= !stat_valid(g[e]);
    if (r < n_lines) bad |= !(g[REC - 1] >= 2.0);
    const bool any = __ballot(bad) != 0ull;
    if (lane_id() == 0) flags[r] = any ? 1 : 0;
}

// ahead[g] = the determinant of the step (line g, line g + 1) of a problem: BIC the union's
// covariance, GLR the count-weighted mean covariance; 0 for the last line of a problem (unread).
// One wave per pair, the left line staged in the wave's own LDS slab.
template <bool TWO>
__global__ __launch_bounds__(MRG_AHEAD_WAVES * WAVE) void k_merge_ahead(
        const double* __restrict__ ex, const double* __restrict__ pk, const int64_t* __restrict__ line_off,
        int64_t n_prob, int64_t n_lines, int kind, double* __restrict__ ahead, int* prob_err) {
    __shared__ double slab[MRG_AHEAD_WAVES][QREC];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    const int64_t g0 = (int64_t)blockIdx.x * MRG_AHEAD_WAVES + wave;
    const int64_t g = g0 < n_lines ? g0 : n_lines - 1;         // (whole waves past the end redo the last line)
    const int p = find_problem(line_off, n_prob, g);
    const bool pair = g0 < n_lines && g + 1 < line_off[p + 1];
    const int64_t gc = pair ? g + 1 : g;
    double* ldsA = slab[wave];
    for (int e = lane; e < QREC; e += WAVE) ldsA[e] = ex[g * QREC + e];
    __syncthreads();
    const QuadLane L = quad_lane();
    const double det = quad_pair_det<TWO>(kind, ldsA, ldsA[QREC_COUNT_AT], ldsA, ex + gc * QREC, pk + gc * REC,
                                          false, L, prob_err + p);
    if (g0 < n_lines && lane == 0) ahead[g] = pair ? det : 0.0;
}

// BIC of a step with the left term frozen: the 5-argument bic keeps
// c1 = 0.5 N1 log det S1 of the first call.  Rounded like finish_distance, whatever surrounds it.
__device__ __forceinline__ double merge_bic_distance(double lambdac, double c1, double nA, double nC, double ldC,
                                                     double ldx) {
#pragma clang fp contract(off)
    const double n = nA + nC;
    double d = 0.5 * n * ldx - c1 - 0.5 * nC * ldC;
    d -= lambdac * 0.5 * PEN_UNIT * log(n);
    return d;
}

// The script's summary counters over one problem, each started where the script starts it and
// moved by its comparisons (as SwTurnStats): windows = steps whose distance is not +-inf,
// detections = merges.
struct MergeStats {
    long long *win_cnt, *det_cnt;
    double *win_max, *win_min, *det_max, *det_min;
};

// One wave per problem p = blockIdx.x, lines line_off[p] .. line_off[p + 1] of the per-line arrays
// (ex / pk: quad and packed records, lines first, gap records behind them; gap_rec[g]: the record
// of the gap behind line g, -1 when it is empty; ld / aux: k_cluster_prep_batch's terms of the
// lines).  L lives in LDS as a quad record.  Step s decides line s:
//   - the left side or the line cannot give a covariance (flags): the problem stops there, its
//     error word is raised; nothing of it touches another problem
//   - the determinant: ahead[s - 1] when L is the unmerged line s - 1 and an ahead pass ran, else
//     quad_pair_det in DPP row 0; with GLR behind a merge row 1 of the same pass takes L's own
//     covariance (its log det is no line's)
//   - distance in fp64 in the script's order, a merge when d < threshold and d is not +-inf
// merged[g] / dist[g]: 0 and NaN for a problem's first line, -1 and NaN behind a stop.
// done[p]: lines decided.  Every loop is bounded by the problem's line count; no waiting on
// other workgroups anywhere.
template <bool TWO>
__global__ __launch_bounds__(WAVE) void k_merge_chain_batch(
        const double* __restrict__ ex, const double* __restrict__ pk, const double* __restrict__ ld,
        const double* __restrict__ aux, const int64_t* __restrict__ line_off, const int32_t* __restrict__ gap_rec,
        const int32_t* __restrict__ flags, const double* __restrict__ ahead, int kind, double lambdac, double threshold,
        int32_t* __restrict__ merged, double* __restrict__ dist, long long* __restrict__ done, MergeStats st,
        int* prob_err, int* err, double* pinv_ws) {
    __shared__ double ldsL[QREC];
    __shared__ double auxL[AUX];
    const int lane = lane_id();
    const QuadLane L = quad_lane();
    const long long p = blockIdx.x, off = line_off[p], n = line_off[p + 1] - off;
    int* perr = prob_err + p;
    long long cnt = 0, ndet = 0;
    double wmax = 0.0, wmin = MAXINT_F, dmax = 0.0, dmin = MAXINT_F;
    long long s = 0;
    if (n > 0) {                                         // (uniform: the workgroup is one wave)
        const bool kl2 = kind == SPKD_KL2;
        bool fresh = true;                               // L is the unmerged line s - 1
        bool bad_left = flags[off] != 0;
        double ldL = ld[off], c1 = 0.0;
        bool have_c1 = false;
        for (int e = lane; e < QREC; e += WAVE) ldsL[e] = ex[off * QREC + e];
        if (lane == 0) { merged[off] = 0; dist[off] = __builtin_nan(""); }
        __syncthreads();
        for (s = 1; s < n; ++s) {
            const long long g = off + s;
            if (bad_left || flags[g] != 0) {
                if (lane == 0) atomicOr(perr, ERR_NONFINITE);
                break;
            }
            const double nA = ldsL[QREC_COUNT_AT], nC = pk[g * REC + REC - 1];
            double d;
            if (kl2) {
                d = kl2_from_aux(fresh ? aux + (g - 1) * AUX : auxL, aux + g * AUX);
            } else {
                double det;
                if (fresh && ahead) {
                    det = ahead[g - 1];
                } else {
                    const bool own = TWO && kind == SPKD_GLR && !fresh;
                    const double v = quad_pair_det<TWO>(kind, ldsL, nA, ldsL, ex + g * QREC, pk + g * REC,
                                                        own && L.m == 1, L, perr);
                    det = __shfl(v, 0);
                    if (own) ldL = log(__shfl(v, 16));
                }
                const double ldx = log(det);
                if (kind == SPKD_BIC) {
                    if (!have_c1) {
#pragma clang fp contract(off)
                        c1 = 0.5 * nA * ldL;
                        have_c1 = true;
                    }
                    d = merge_bic_distance(lambdac, c1, nA, nC, ld[g], ldx);
                } else {
                    d = finish_distance(kind, lambdac, nA, ldL, nC, ld[g], ldx);
                }
            }
            __syncthreads();
            if (*reinterpret_cast<volatile int*>(perr) & ERR_NONFINITE) break;
            const bool inf = fabs(d) == __builtin_huge_val();
            if (!inf) {
                ++cnt;
                if (d > wmax) wmax = d;
                if (d < wmin) wmin = d;
            }
            const bool join = d < threshold && !inf;
            if (lane == 0) { merged[g] = join ? 1 : 0; dist[g] = d; }
            if (join) {
                ++ndet;
                if (d > dmax) dmax = d;
                if (d < dmin) dmin = d;
                const long long gr = gap_rec[g - 1];
                if (gr >= 0) bad_left = flags[gr] != 0;
                for (int e = lane; e < QREC; e += WAVE) {
                    double v = ldsL[e];
                    if (gr >= 0) v += ex[gr * QREC + e];
                    ldsL[e] = v + ex[g * QREC + e];
                }
                fresh = false;
                __syncthreads();
                if (kl2) {
                    kl2_aux_from_qr(ldsL, auxL, pinv_ws);
                    __syncthreads();
                }
            } else {
                for (int e = lane; e < QREC; e += WAVE) ldsL[e] = ex[g * QREC + e];
                ldL = ld[g];
                fresh = true;
                __syncthreads();
            }
        }
    }
    for (long long r = s + lane; r < n; r += WAVE) { merged[off + r] = -1; dist[off + r] = __builtin_nan(""); }
    if (lane == 0) {
        done[p] = s;
        st.win_cnt[p] = cnt;
        st.win_max[p] = wmax;
        st.win_min[p] = wmin;
        st.det_cnt[p] = ndet;
        st.det_max[p] = dmax;
        st.det_min[p] = dmin;
        const int e = *reinterpret_cast<volatile int*>(perr);
        if (e) atomicOr(err, e);
    }
}

}  // namespace spkd
