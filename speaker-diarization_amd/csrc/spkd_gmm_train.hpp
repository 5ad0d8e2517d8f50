// Diagonal-covariance mixture speaker models trained by EM on the device (spkd_gmm_train) and the
// per-frame log-likelihoods under them (spkd_gmm_loglik_seq): the GMM form of the resegmentation
// stage's scoring half.
// PARITY: no reference counterpart -- the reference stops at clustering; tests/reseg_gmm_numpy.py
// restates the initial model, one EM step and the scores in numpy.
//
// A speaker's frames are the frames of its ranges in the caller's order, numbered 0 .. N - 1; that
// numbering is cut into tiles of GT_TILE ordinals and chunks of GT_CHUNK_TILES tiles, whatever the
// grid and whoever else is in the call.  Every sum below is one chain in ordinal order (inside a
// chunk) and then in chunk order: no atomics, no cross-lane reduction of a partial sum, so a
// speaker's model has the same bits in every run, alone or among others.
//
//   k_gmm_estep<HARD> : one wave per (speaker, chunk).  A tile's frames are found by a binary search of
//                       the speaker's ranges (a lane per frame), staged through LDS with coalesced
//                       loads (ranges that are contiguous in memory load contiguously) and used twice:
//                       phase 1, a lane per frame: the K responsibilities g_k and the frame's
//                         log-likelihood go to LDS.  The model's address is wave-uniform: scalar
//                         loads, the FMAs take means and inverse variances from SGPRs.  HARD: g_k is
//                         1 for the component whose slot [floor(kN/K), floor((k+1)N/K)) holds the
//                         ordinal, else 0 -- the pass behind the initial model and the variance floor.
//                       phase 2, a lane per dimension (lane 39 a column of ones): the tile's frames in
//                         order, A_k += g_k x, B_k += g_k x^2 in 2 K registers; lane 39's A_k is G_k.
//                         Every lane adds up the log-likelihoods L (the same chain in each).
//                       The chunk's partials go to global memory.
//   k_gmm_mstep       : one wave per speaker.  Adds the chunk partials in chunk order and forms the
//                       model: ln w, mean, 1 / var, log_norm per component (a lane per dimension; the
//                       39 ln var of log_norm are added in dimension order through LDS).
//   k_gmm_loglik_seq  : k_gauss_loglik's shape: one wave per tile of one sequence, a lane per frame,
//                       the frame in registers, the loop over the sequence's speakers not unrolled.
//                       The K component log-likelihoods of a frame wait in LDS for their maximum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_gauss.hpp"

namespace spkd {

constexpr int GT_COMP = 80;           // doubles per component: ln w, mean[39], 1 / var[39], log_norm (SPKD_GMM_COMP)
constexpr int GT_MAX_COMP = 8;        // components per speaker (SPKD_GMM_MAX_COMP)
constexpr int GT_TILE = 64;           // frame ordinals per tile, one lane each (SPKD_GMM_TILE)
constexpr int GT_CHUNK_TILES = 16;    // tiles per chunk, the unit of a partial sum (SPKD_GMM_CHUNK_TILES)
constexpr int GT_CHUNK = GT_TILE * GT_CHUNK_TILES;
constexpr int GT_MEAN = 1, GT_IVAR = 1 + D, GT_NORM = GT_COMP - 1;
constexpr int GT_MIN_PER_COMP = D + 1;      // a speaker of fewer than 40 K frames is not modelled
constexpr int GT_B = D + 1;           // a chunk's partials of one component: A[39], G, B[39], G again
constexpr double GT_LN_2PI = 1.8378770664093453;
static_assert(GT_TILE == GS_TILE, "one tile for both models: spkd_gauss.hpp's, a lane per frame");
static_assert(2 + 2 * D == GT_COMP && 2 * GT_B == GT_COMP, "ln w, mean, 1 / var, log_norm");

__device__ inline bool gt_finite(double v) { return fabs(v) < INFINITY; }

// the absolute frame of ordinal o of a speaker that owns the ranges [r0, r1): ord[r] is the ordinal
// of range r's first frame; the last range that starts at or before o holds it (o < N, so that range
// is not empty)
__device__ inline long long gt_frame(const long long* __restrict__ ord, const long long* __restrict__ begin,
                                     long long r0, long long r1, long long o) {
    long long lo = r0, hi = r1 - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (ord[mid] <= o) lo = mid; else hi = mid - 1;
    }
    return begin[lo] + (o - ord[lo]);
}

// the frames of the tile of ordinals [o0, o0 + len) of the speaker that owns the ranges [r0, r1), staged
// in xs (fr: the tile's absolute frames): a lane per frame finds it, then coalesced loads
__device__ inline void gt_stage_tile(const float* __restrict__ frames, const long long* __restrict__ range_ord,
                                     const long long* __restrict__ range_begin, long long r0, long long r1,
                                     long long o0, int len, int lane, long long* fr, float* xs) {
    if (lane < len) fr[lane] = gt_frame(range_ord, range_begin, r0, r1, o0 + lane);
    __syncthreads();
    constexpr int PF = (GT_TILE * D + WAVE - 1) / WAVE;              // 39 floats a lane
#pragma unroll 13
    for (int k = 0; k < PF; ++k) {
        const int idx = lane + WAVE * k;
        if (idx < len * D) {
            const int j = idx / D;
            xs[idx] = frames[fr[j] * D + (idx - j * D)];
        }
    }
    __syncthreads();
}

// the lane's frame x under the K components of M (a wave-uniform address): the log-likelihood of every
// live component (one whose ln w is not -inf; the others take no part) to lk[k * GT_TILE + lane]; returns
// their maximum
__device__ inline double gt_component_logliks(const float (&x)[D], const double* __restrict__ M, int K, int lane,
                                              double* lk) {
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const double* __restrict__ Mk = M + k * GT_COMP;
        if (Mk[0] == -INFINITY) continue;                   // (wave-uniform) contributes nothing
        double q = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const double d = (double)x[j] - Mk[GT_MEAN + j];
            q = fma(d * d, Mk[GT_IVAR + j], q);
        }
        lk[k * GT_TILE + lane] = fma(-0.5, q, Mk[0] + Mk[GT_NORM]);
    }
    double m = -INFINITY;
#pragma unroll 1
    for (int k = 0; k < K; ++k)
        if (M[k * GT_COMP] != -INFINITY) {
            const double l = lk[k * GT_TILE + lane];
            if (l > m) m = l;
        }
    return m;
}

// phase 1 of a soft pass, the lane's frame of the staged tile under the K components of M: its
// responsibilities g_k to gl[k * GT_TILE + lane] (0 for a component that is not live), its log-likelihood
// to lls[lane]
__device__ inline void gt_responsibilities(const float* xs, const double* __restrict__ M, int K, int lane,
                                           double* gl, double* lls) {
    float x[D];
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = xs[lane * D + j];
    const double m = gt_component_logliks(x, M, K, lane, gl);
    double sum = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        double e = 0.0;
        if (M[k * GT_COMP] != -INFINITY) {
            e = exp(gl[k * GT_TILE + lane] - m);
            sum += e;
        }
        gl[k * GT_TILE + lane] = e;
    }
#pragma unroll 1
    for (int k = 0; k < K; ++k) gl[k * GT_TILE + lane] /= sum;
    lls[lane] = m + log(sum);
}

template <bool HARD>
__global__ __launch_bounds__(WAVE) void k_gmm_estep(
        const float* __restrict__ frames, const long long* __restrict__ range_begin,
        const long long* __restrict__ range_ord, const long long* __restrict__ set_off,
        const long long* __restrict__ spk_n, const int* __restrict__ chunk_spk, const int* __restrict__ chunk_idx,
        const double* __restrict__ gmm, int K, double* __restrict__ part, double* __restrict__ part_ll) {
    __shared__ float xs[GT_TILE * D];
    __shared__ double gl[GT_MAX_COMP * GT_TILE];
    __shared__ double lls[GT_TILE];
    __shared__ long long fr[GT_TILE];
    const int lane = threadIdx.x;
    const long long wg = blockIdx.x;
    const int s = chunk_spk[wg];
    const long long N = spk_n[s], r0 = set_off[s], r1 = set_off[s + 1];
    const long long c0 = (long long)chunk_idx[wg] * GT_CHUNK;
    const double* __restrict__ M = gmm + (long long)s * K * GT_COMP;
    double A[GT_MAX_COMP], B[GT_MAX_COMP];
#pragma unroll
    for (int k = 0; k < GT_MAX_COMP; ++k) A[k] = B[k] = 0.0;
    double L = 0.0;
    for (int t = 0; t < GT_CHUNK_TILES; ++t) {
        const long long o0 = c0 + (long long)t * GT_TILE;
        if (o0 >= N) break;                                             // (wave-uniform)
        const int len = N - o0 < GT_TILE ? (int)(N - o0) : GT_TILE;
        gt_stage_tile(frames, range_ord, range_begin, r0, r1, o0, len, lane, fr, xs);
        if (lane < len) {
            if (HARD) {
                const long long o = o0 + lane;
                for (int k = 0; k < K; ++k)
                    gl[k * GT_TILE + lane] = (o >= k * N / K && o < (k + 1) * N / K) ? 1.0 : 0.0;
                lls[lane] = 0.0;
            } else {
                gt_responsibilities(xs, M, K, lane, gl, lls);
            }
        }
        __syncthreads();
        for (int j = 0; j < len; ++j) {
            const double x = lane < D ? (double)xs[j * D + lane] : 1.0;
            const double x2 = x * x;
#pragma unroll
            for (int k = 0; k < GT_MAX_COMP; ++k)
                if (k < K) {                                            // (wave-uniform)
                    const double g = gl[k * GT_TILE + j];
                    A[k] = fma(g, x, A[k]);
                    B[k] = fma(g, x2, B[k]);
                }
            L += lls[j];
        }
        __syncthreads();
    }
    double* __restrict__ P = part + wg * K * GT_COMP;
#pragma unroll
    for (int k = 0; k < GT_MAX_COMP; ++k)
        if (k < K && lane < GT_B) {
            P[k * GT_COMP + lane] = A[k];
            P[k * GT_COMP + GT_B + lane] = B[k];
        }
    if (lane == 0) part_ll[wg] = L;
}

// init: the partials are a hard pass's.  V_d, the ML variance of all the speaker's frames, gives the
// floor var_floor V_d (kept in floor_v for the call's later steps) and, with N >= 40 K, the first
// ok; the model is written when write_model (from_model = 0).  Otherwise an EM step: the log-
// likelihood of the model that entered it goes to loglik[s * n_iter + iter], the model is replaced.
__global__ __launch_bounds__(WAVE) void k_gmm_mstep(
        const double* __restrict__ part, const double* __restrict__ part_ll, const long long* __restrict__ chunk_off,
        const long long* __restrict__ spk_n, int K, int init, int write_model, double var_floor, int iter, int n_iter,
        double* gmm, double* floor_v, int* ok, double* loglik) {
    __shared__ double lv[WAVE];
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const long long c0 = chunk_off[s], c1 = chunk_off[s + 1];
    const double N = (double)spk_n[s];
    const int KC = K * GT_COMP;
    double* M = gmm + s * KC;
    const int col = lane < GT_B ? lane : 0;                             // (lanes past 39 repeat lane 0)
    bool fin = true, good = true;
    double fl = 0.0;
    if (init) {
        double ta = 0.0, tb = 0.0;
        for (int k = 0; k < K; ++k) {
            double a = 0.0, b = 0.0;
            for (long long c = c0; c < c1; ++c) {
                a += part[c * KC + k * GT_COMP + col];
                b += part[c * KC + k * GT_COMP + GT_B + col];
            }
            fin = fin && gt_finite(a) && gt_finite(b);
            ta += a;
            tb += b;
        }
        const double mu = ta / N;
        const double V = tb / N - mu * mu;
        good = spk_n[s] >= (long long)GT_MIN_PER_COMP * K && __all(lane >= D || (V > 0.0 && V < INFINITY));
        fl = var_floor * V;
        floor_v[s * WAVE + lane] = fl;
    } else {
        fl = floor_v[s * WAVE + lane];
        double L = 0.0;
        for (long long c = c0; c < c1; ++c) L += part_ll[c];
        fin = gt_finite(L);
        if (lane == 0) loglik[s * n_iter + iter] = L;
    }
    if (!init || write_model) {
#pragma unroll 1
        for (int k = 0; k < K; ++k) {
            double a = 0.0, b = 0.0;
            for (long long c = c0; c < c1; ++c) {
                a += part[c * KC + k * GT_COMP + col];
                b += part[c * KC + k * GT_COMP + GT_B + col];
            }
            fin = fin && gt_finite(a) && gt_finite(b);
            const double G = __shfl(a, D);                              // lane 39's column of ones
            double mean, iv, lnv = 0.0, norm;
            const bool moves = G >= 2.0;                                // (wave-uniform)
            if (moves) {
                mean = a / G;
                double v = b / G - mean * mean;
                if (v < fl) v = fl;
                iv = 1.0 / v;
                lnv = log(v);
            } else {
                mean = init ? 0.0 : M[k * GT_COMP + GT_MEAN + (lane < D ? lane : 0)];
                iv = init ? 1.0 : M[k * GT_COMP + GT_IVAR + (lane < D ? lane : 0)];
            }
            lv[lane] = lane < D ? lnv : 0.0;
            __syncthreads();
            double sl = 0.0;
            for (int d = 0; d < D; ++d) sl += lv[d];                    // (in dimension order, the same in every lane)
            __syncthreads();
            norm = moves ? -0.5 * (D * GT_LN_2PI + sl) : (init ? -0.5 * D * GT_LN_2PI : M[k * GT_COMP + GT_NORM]);
            // a model that cannot score (a variance of 0 under a floor of 0) is not ok either
            fin = fin && (lane >= D || (gt_finite(mean) && gt_finite(iv) && iv > 0.0)) && gt_finite(norm);
            if (lane < D) {
                M[k * GT_COMP + GT_MEAN + lane] = mean;
                M[k * GT_COMP + GT_IVAR + lane] = iv;
            }
            if (lane == 0) {
                M[k * GT_COMP] = log(G / N);
                M[k * GT_COMP + GT_NORM] = norm;
            }
        }
    }
    const bool all_fin = __all(fin);
    if (lane == 0) ok[s] = ((init || ok[s]) && good && all_fin) ? 1 : 0;
}

__global__ __launch_bounds__(WAVE) void k_gmm_loglik_seq(
        const float* __restrict__ frames, const double* __restrict__ gmm, int K, const int* __restrict__ model_ok,
        const long long* __restrict__ seq_begin, const long long* __restrict__ seq_end,
        const long long* __restrict__ seq_row, const long long* __restrict__ seq_tile,
        const int* __restrict__ seq_model, const int* __restrict__ seq_n_models,
        const int* __restrict__ tile_seq, int n_cols, float* __restrict__ scores) {
    __shared__ float xs[GT_TILE * D];
    __shared__ float so[GT_TILE * GS_MAX_COLS];
    __shared__ double lk[GT_MAX_COMP * GT_TILE];
    const int lane = threadIdx.x;
    float x[D];
    const SeqTile t = gs_stage_tile(frames, seq_begin, seq_end, seq_row, seq_tile, seq_model, seq_n_models, tile_seq, lane, xs, x);
#pragma unroll 1
    for (int m = 0; m < n_cols; ++m) {
        float sc = -INFINITY;
        if (m < t.nm && model_ok[t.m0 + m]) {                      // (wave-uniform)
            const double* __restrict__ M = gmm + (long long)(t.m0 + m) * K * GT_COMP;
            const double mx = gt_component_logliks(x, M, K, lane, lk);
            double sum = 0.0;
#pragma unroll 1
            for (int k = 0; k < K; ++k)
                if (M[k * GT_COMP] != -INFINITY) sum += exp(lk[k * GT_TILE + lane] - mx);
            sc = (float)(mx + log(sum));
        }
        so[lane * n_cols + m] = sc;
    }
    gs_store_tile(t, so, n_cols, lane, scores);
}

}  // namespace spkd
