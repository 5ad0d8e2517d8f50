// K_post_stats: frames and frame posteriors -> posterior-weighted statistics records
// (spkd_post_stats): record m = sum over the frames t of the sequences that model m covers of
// w_t(m) [x_t; 1] [x_t; 1]^T, w the float32 posterior of m at t.  Baum-Welch retraining of the
// speakers of resegmentation: spkd_fb_posterior_batch in front, spkd_gauss_models behind.
//
// The shape of K_stats (spkd_stats.hpp), whose pieces it is made of:
//   k_post_chunk_stats : one workgroup per (chunk of <= STATS_CHUNK frames of one sequence, column);
//                        chunk_stats_accumulate with the four xi of a lane's block scaled by the
//                        frame's weight ahead of its 16 FMAs -- 820 FMAs a frame and column, as
//                        k_chunk_stats spends on a frame.  A frame whose weight is exactly 0 is
//                        passed over: it adds nothing whatever it holds, and a decoder's posteriors
//                        are 0 on most frames of most columns;
//   k_reduce_sets      : per model, the sum of its partials -- the host hands a model's workgroups
//                        consecutive slots, in the order (sequence of the call, chunk), so the bits of
//                        a record depend on nothing but the model's own sequences.
// The columns of a chunk read the same frames again, from L2 or the Infinity Cache: 156 B a frame
// against 820 FMAs.  Algorithmic bytes: (156 + 4) B per frame and column read, 6 560 B per workgroup
// written and read again, 6 560 B per model written.
#pragma once
#include "spkd_stats.hpp"

namespace spkd {

struct PostItem {
    int64_t begin;      // first frame
    int64_t row;        // its row of the posteriors
    int64_t slot;       // the partial record it writes
    int32_t len;        // frames in the chunk
    int32_t col;        // column of the posteriors
};

// the weights of a tile: fetched with the tile's frames (a register of the first STATS_TILE
// threads), converted once, read by every wave as a broadcast
struct PostWeight {
    const float* __restrict__ w;         // the column's posterior at the chunk's first frame
    int stride;                          // n_cols
    double (&ws)[STATS_TILE];
    float next = 0.0f;
    __device__ __forceinline__ PostWeight(const float* w_, int stride_, double (&ws_)[STATS_TILE])
        : w(w_), stride(stride_), ws(ws_) {}
    __device__ __forceinline__ void issue(int t0, int tl) {
        const int tid = threadIdx.x;
        if (tid < STATS_TILE) next = tid < tl ? w[(int64_t)(t0 + tid) * stride] : 0.0f;
    }
    __device__ __forceinline__ void stage() {
        if (threadIdx.x < STATS_TILE) ws[threadIdx.x] = (double)next;
    }
    __device__ __forceinline__ bool skip(int f) const { return ws[f] == 0.0; }
    __device__ __forceinline__ void scale(int f, double (&xi)[SB]) const {
        const double v = ws[f];
#pragma unroll
        for (int a = 0; a < SB; ++a) xi[a] *= v;
    }
};

__global__ __launch_bounds__(STATS_TPB) void k_post_chunk_stats(
        const float* __restrict__ frames, const float* __restrict__ post, const PostItem* __restrict__ items,
        int n_cols, double* __restrict__ partial) {
    __shared__ double xs[STATS_TILE][DA];                       // 20 KB
    __shared__ double part[STATS_WAVES][SBLOCKS][SB * SB];      // 28 KB
    __shared__ double ws[STATS_TILE];
    const PostItem it = items[blockIdx.x];
    double* out = partial + it.slot * REC;
    chunk_stats_accumulate(frames, it.begin, it.len, xs, part, [&](int, int e, double v) { out[e] = v; },
                           PostWeight(post + it.row * n_cols + it.col, n_cols, ws));
}

}  // namespace spkd
