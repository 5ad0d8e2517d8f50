// Full-covariance Gaussian speaker models and their per-frame log-likelihoods (spkd_gauss_models,
// spkd_gauss_loglik): the scoring half of a Viterbi resegmentation of a batch's speakers.
// PARITY: no reference counterpart -- the reference stops at clustering; tests/reseg_numpy.py
// restates both kernels in numpy.
//
//   k_gauss_models : one wave per statistics record.  The record goes to LDS, the unbiased
//                    covariance S (cov_rows' form: M_ij - (s_i / n) s_j, times 1 / (n - 1)) is
//                    written as a 39 x 39 lower triangle, factored S = L L^T in place (right-looking,
//                    lane i owns row i, one column a step) and inverted by forward substitution,
//                    lane c owning column c of W = L^-1.  A pivot counts as positive when it is
//                    finite and above GS_PIVOT_REL of the diagonal entry it started from
//                    (M_jj / (n - 1)): what cancellation leaves of a constant stretch, or of the
//                    rank a set of fewer than 40 frames cannot have, is rounding noise, not a pivot.
//                    39^3 / 3 FMAs a record: the work is the speakers', not the frames'.
//   k_gauss_loglik : one wave per tile of GS_TILE frames of one sequence, a lane per frame.  The
//                    tile's 39-float frames are contiguous in memory: they are staged through LDS
//                    with coalesced loads and read back at a stride of 39 floats, which is odd, so
//                    conflict-free.  A lane keeps its frame in registers and walks the sequence's
//                    models one after the other: d = x - mu (39 doubles in registers), y_i = sum_{j
//                    <= i} W_ij d_j, score = c - 1/2 sum y_i^2, 780 + 78 fp64 FMAs a model.  The
//                    model is the same for every lane of the wave and its address is formed from
//                    wave-uniform values only: the compiler reads it with scalar loads and the
//                    FMAs take W_ij from SGPRs -- no LDS traffic and no vector load in the loop.
//                    The scores of a tile are collected in LDS and leave in one coalesced store
//                    of len x n_cols floats (the compact [sum len][n_cols] layout is contiguous
//                    per tile).  All fp64 from the float32 frame, rounded once on the store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"

namespace spkd {

constexpr int GS_TILE = 64;           // frames per tile, one lane each (SPKD_GAUSS_TILE)
constexpr int GS_MODEL = 820;         // doubles per model: mu[39], W packed lower row-major [780], c (SPKD_GAUSS_MODEL)
constexpr int GS_W = D;               // offset of W in a model
constexpr int GS_C = GS_MODEL - 1;    // offset of c
constexpr int GS_MAX_COLS = 16;
constexpr int GS_MIN_FRAMES = D + 1;  // below: the covariance has no full rank
constexpr double GS_PIVOT_REL = 0x1p-40;
constexpr int GS_LD = D + 2;          // row stride of the LDS triangles
static_assert(GS_TILE == WAVE, "a lane per frame of the tile");
static_assert(D + D * (D + 1) / 2 + 1 == GS_MODEL, "mu, W, c");

__host__ __device__ constexpr int gs_w(int i, int j) { return GS_W + i * (i + 1) / 2 + j; }   // j <= i

__global__ __launch_bounds__(WAVE) void k_gauss_models(
        const double* __restrict__ stats, double* __restrict__ models, int* __restrict__ ok) {
    __shared__ double rec[REC];
    __shared__ double A[D][GS_LD];       // S, then L, lower triangle
    __shared__ double Wm[D][GS_LD];      // L^-1, lower triangle
    const int lane = threadIdx.x;
    const long long r = blockIdx.x;
    stage1(rec, stats + r * REC);
    __syncthreads();
    const double cnt = rec[pk(D, D)];
    const double inv_n = 1.0 / cnt, f = 1.0 / (cnt - 1.0);
    if (lane < D) {
        const double mi = -(rec[pk(lane, D)] * inv_n);
        for (int j = 0; j <= lane; ++j) A[lane][j] = fma(mi, rec[pk(j, D)], rec[pk(j, lane)]) * f;
    }
    __syncthreads();
    bool good = cnt >= (double)GS_MIN_FRAMES && cnt < INFINITY;
    double logsum = 0.0;
    for (int j = 0; j < D; ++j) {
        const double dj = A[j][j];                                 // (the same for every lane)
        good = good && dj > GS_PIVOT_REL * (rec[pk(j, j)] * f) && dj < INFINITY;
        const double l = sqrt(dj);
        logsum += log(l);
        double lij = 0.0;
        if (lane > j && lane < D) lij = A[lane][j] / l;
        __syncthreads();
        if (lane > j && lane < D) A[lane][j] = lij;
        if (lane == j) A[j][j] = l;
        __syncthreads();
        if (lane > j && lane < D)
            for (int k = j + 1; k <= lane; ++k) A[lane][k] = fma(-lij, A[k][j], A[lane][k]);
        __syncthreads();
    }
    if (lane < D) {                                                // column `lane` of L^-1
        const int c = lane;
        Wm[c][c] = 1.0 / A[c][c];
        for (int i = c + 1; i < D; ++i) {
            double s = 0.0;
            for (int k = c; k < i; ++k) s = fma(A[i][k], Wm[k][c], s);
            Wm[i][c] = -s / A[i][i];
        }
    }
    __syncthreads();
    double* out = models + r * GS_MODEL;
    if (lane < D) out[lane] = rec[pk(lane, D)] * inv_n;
    for (int i = 0; i < D; ++i)
        if (lane <= i) out[gs_w(i, lane)] = Wm[i][lane];
    if (lane == 0) {
        out[GS_C] = -0.5 * D * 1.8378770664093453 - logsum;         // ln 2 pi
        ok[r] = good ? 1 : 0;
    }
}

// The tile of a workgroup of the scoring kernels (k_gauss_loglik, k_gmm_loglik_seq; the table is the host's
// SeqTable): its frames, the first of its rows of the scores, its sequence's first model and model count.
// All of it comes from blockIdx and the table, so it is wave-uniform, and so is a model's address formed from it.
struct SeqTile {
    int len;                              // >= 1: the host counts the tiles
    long long row0;
    int m0, nm;
};

// finds the workgroup's tile, stages its len * D floats in xs and leaves the lane's frame in x (zeros past len)
__device__ inline SeqTile gs_stage_tile(
        const float* __restrict__ frames, const long long* __restrict__ seq_begin, const long long* __restrict__ seq_end,
        const long long* __restrict__ seq_row, const long long* __restrict__ seq_tile,
        const int* __restrict__ seq_model, const int* __restrict__ seq_n_models,
        const int* __restrict__ tile_seq, int lane, float* xs, float (&x)[D]) {
    const long long tile = blockIdx.x;
    const int q = tile_seq[tile];
    const long long t0 = (tile - seq_tile[q]) * GS_TILE;
    const long long b = seq_begin[q] + t0;
    const long long left = seq_end[q] - b;
    const SeqTile t = {left < GS_TILE ? (int)left : GS_TILE, seq_row[q] + t0, seq_model[q], seq_n_models[q]};
    const float* src = frames + b * D;
    constexpr int PF = (GS_TILE * D + WAVE - 1) / WAVE;              // 39 floats a lane
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int idx = lane + WAVE * k;
        if (idx < t.len * D) xs[idx] = src[idx];
    }
    __syncthreads();
    const bool has = lane < t.len;
#pragma unroll
    for (int j = 0; j < D; ++j) x[j] = has ? xs[lane * D + j] : 0.0f;
    return t;
}

// the tile's len * n_cols scores from so (row `lane`, column m at so[lane * n_cols + m]) in one coalesced store
__device__ inline void gs_store_tile(const SeqTile& t, const float* so, int n_cols, int lane, float* __restrict__ scores) {
    __syncthreads();
    float* dst = scores + t.row0 * n_cols;
    for (int idx = lane; idx < t.len * n_cols; idx += WAVE) dst[idx] = so[idx];
}

__global__ __launch_bounds__(WAVE) void k_gauss_loglik(
        const float* __restrict__ frames, const double* __restrict__ models, const int* __restrict__ model_ok,
        const long long* __restrict__ seq_begin, const long long* __restrict__ seq_end,
        const long long* __restrict__ seq_row, const long long* __restrict__ seq_tile,
        const int* __restrict__ seq_model, const int* __restrict__ seq_n_models,
        const int* __restrict__ tile_seq, int n_cols, float* __restrict__ scores) {
    __shared__ float xs[GS_TILE * D];
    __shared__ float so[GS_TILE * GS_MAX_COLS];
    const int lane = threadIdx.x;
    float x[D];
    const SeqTile t = gs_stage_tile(frames, seq_begin, seq_end, seq_row, seq_tile, seq_model, seq_n_models, tile_seq, lane, xs, x);
#pragma unroll 1
    for (int m = 0; m < n_cols; ++m) {
        float s = -INFINITY;
        if (m < t.nm && model_ok[t.m0 + m]) {                      // (wave-uniform)
            const double* __restrict__ M = models + (long long)(t.m0 + m) * GS_MODEL;
            double d[D];
#pragma unroll
            for (int j = 0; j < D; ++j) d[j] = (double)x[j] - M[j];
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double y = M[gs_w(i, 0)] * d[0];
#pragma unroll
                for (int j = 1; j <= i; ++j) y = fma(M[gs_w(i, j)], d[j], y);
                acc = fma(y, y, acc);
            }
            s = (float)fma(-0.5, acc, M[GS_C]);
        }
        so[lane * n_cols + m] = s;
    }
    gs_store_tile(t, so, n_cols, lane, scores);
}

}  // namespace spkd
