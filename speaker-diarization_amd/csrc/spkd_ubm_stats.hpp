// Zeroth- and first-order statistics of every speaker's frames under one universal background model
// (spkd_ubm_stats): what linking by cross-likelihood ratio (spkd_clr.hpp) compares and adds.
// PARITY: no reference counterpart -- the reference links nothing across files; tests/link_clr_numpy.py
// restates the records in numpy.
//
// The partition and the order of every sum are spkd_gmm_train.hpp's: a speaker's frames are numbered in
// range order, cut into tiles of GT_TILE ordinals and chunks of GT_CHUNK_TILES tiles; a chunk is one
// chain in ordinal order, the chunks are added in chunk order, no atomics.  The tile staging and the
// responsibilities are that file's device functions, with the one UBM as every speaker's model.
//
//   k_ubm_estep  : one wave per (speaker, chunk).  Phase 1, a lane per frame: the C responsibilities to
//                  LDS (gt_responsibilities).  Phase 2, a lane per column of the record (lane 0 a column
//                  of ones, lane 1 + d dimension d): the tile's frames in order, S_c += g_c x in C
//                  registers.  The chunk's partials go to global memory; a frame is read once.
//   k_ubm_reduce : one wave per speaker.  Adds the chunk partials in chunk order, writes the record
//                  (BW_COMP doubles per component: n_c, f_c[39]) and ok: a frame and every sum finite.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_gmm_train.hpp"

namespace spkd {

constexpr int BW_COMP = 40;           // doubles per component of a speaker record: n_c, f_c[39] (SPKD_BW_COMP)
static_assert(BW_COMP == D + 1 && BW_COMP <= WAVE, "a lane per column of the record");

__global__ __launch_bounds__(WAVE) void k_ubm_estep(
        const float* __restrict__ frames, const long long* __restrict__ range_begin,
        const long long* __restrict__ range_ord, const long long* __restrict__ set_off,
        const long long* __restrict__ spk_n, const int* __restrict__ chunk_spk, const int* __restrict__ chunk_idx,
        const double* __restrict__ ubm, int K, double* __restrict__ part) {
    __shared__ float xs[GT_TILE * D];
    __shared__ double gl[GT_MAX_COMP * GT_TILE];
    __shared__ double lls[GT_TILE];
    __shared__ long long fr[GT_TILE];
    const int lane = threadIdx.x;
    const long long wg = blockIdx.x;
    const int s = chunk_spk[wg];
    const long long N = spk_n[s], r0 = set_off[s], r1 = set_off[s + 1];
    const long long c0 = (long long)chunk_idx[wg] * GT_CHUNK;
    double S[GT_MAX_COMP];
#pragma unroll
    for (int k = 0; k < GT_MAX_COMP; ++k) S[k] = 0.0;
    for (int t = 0; t < GT_CHUNK_TILES; ++t) {
        const long long o0 = c0 + (long long)t * GT_TILE;
        if (o0 >= N) break;                                             // (wave-uniform)
        const int len = N - o0 < GT_TILE ? (int)(N - o0) : GT_TILE;
        gt_stage_tile(frames, range_ord, range_begin, r0, r1, o0, len, lane, fr, xs);
        if (lane < len) gt_responsibilities(xs, ubm, K, lane, gl, lls);
        __syncthreads();
        const int col = lane >= 1 && lane < BW_COMP ? lane - 1 : 0;     // (lanes past the record repeat dimension 0)
        for (int j = 0; j < len; ++j) {
            const double x = lane == 0 ? 1.0 : (double)xs[j * D + col];
#pragma unroll
            for (int k = 0; k < GT_MAX_COMP; ++k)
                if (k < K) S[k] = fma(gl[k * GT_TILE + j], x, S[k]);    // (wave-uniform)
        }
        __syncthreads();
    }
    double* __restrict__ P = part + wg * K * BW_COMP;
#pragma unroll
    for (int k = 0; k < GT_MAX_COMP; ++k)
        if (k < K && lane < BW_COMP) P[k * BW_COMP + lane] = S[k];
}

__global__ __launch_bounds__(WAVE) void k_ubm_reduce(
        const double* __restrict__ part, const long long* __restrict__ chunk_off, const long long* __restrict__ spk_n,
        int K, double* __restrict__ bw, int* __restrict__ ok) {
    const int lane = threadIdx.x;
    const long long s = blockIdx.x;
    const long long c0 = chunk_off[s], c1 = chunk_off[s + 1];
    const int KC = K * BW_COMP;
    const int col = lane < BW_COMP ? lane : 0;
    bool fin = true;
    for (int k = 0; k < K; ++k) {
        double a = 0.0;
        for (long long c = c0; c < c1; ++c) a += part[c * KC + k * BW_COMP + col];
        fin = fin && gt_finite(a);
        if (lane < BW_COMP) bw[s * KC + k * BW_COMP + lane] = a;
    }
    const bool all_fin = __all(fin);
    if (lane == 0) ok[s] = (spk_n[s] > 0 && all_fin) ? 1 : 0;
}

}  // namespace spkd
