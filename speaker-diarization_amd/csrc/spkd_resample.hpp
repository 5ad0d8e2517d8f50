// Sample-rate conversion and downmix of a batch's audio (spkd_resample_batch): interleaved int16
// files of any mixture of rates and channel counts -> mono int16 at one rate, laid out as
// spkd_mfcc_batch reads it.  The stage `ffmpeg -ar 16000 -ac 1` is for the reference
// (spk-diarization2.py:83).  PARITY UNPINNED (ffmpeg is not available): the filter is the documented
// choice of include/spkd.h, designed on the host (frontend.resample_taps) and handed over as a table.
//
//   k_resample : workgroup per RS_TILE output samples of one file (a tile never crosses a file; the
//                file is found by mf_file_of on the block index).  The tile's input span -- its
//                ceil(TILE down / up) + 2 half frames, zero outside the file -- is downmixed once
//                into LDS as int32 channel sums; with it the conversion's float32 table when both
//                fit RS_LDS_MAX (row stride 2 half + 1: neighbouring lanes sit `down mod up` rows
//                apart, an odd stride keeps them on different banks), else the rows are read from
//                global memory.  Output n of the file: i = n down div up, phase = n down mod up,
//                acc = sum_k (double)h[phase][k] * s[i + k] in fp64, k ascending -- every product is
//                exact (24 x 19 bits), so the fused multiply-add is the restatement's multiply and
//                add -- then rint(acc / channels), saturated.  up == down == 1 is the identity
//                conversion: the downmix alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_mfcc_batch.hpp"

namespace spkd {

constexpr int RS_TILE = 2048;            // output samples per workgroup (SPKD_RESAMPLE_TILE)
constexpr int RS_TPB = 1024;             // 16 waves: a tile whose table takes half the LDS still has 4 waves a SIMD
constexpr int RS_MAX_CH = 8;
constexpr int RS_MAX_HALF = 256;
constexpr int RS_MAX_TERM = 1 << 20;     // up, down: phase + (RS_TILE - 1) * down stays below 2^32
constexpr int RS_MAX_TAPS = 1 << 22;     // floats of one table
constexpr int RS_LDS_MAX = 160 * 1024;   // a CU's LDS
static_assert((long long)RS_MAX_TERM + (long long)(RS_TILE - 1) * RS_MAX_TERM < (1ll << 32), "a tile's phases fit 32 bits");

// input frames a tile of the conversion reads: the span between its first and last output instant and
// the half_taps - 1 / half_taps frames to either side
__host__ __device__ constexpr long long rs_span(long long up, long long down, long long half) {
    return (RS_TILE * down + up - 1) / up + 2 * half;
}
constexpr long long RS_MAX_SPAN = rs_span(1, RS_MAX_HALF / 16, RS_MAX_HALF) + 1;
static_assert(RS_MAX_SPAN * sizeof(int) <= RS_LDS_MAX, "the widest span fits the LDS");

struct RsConv {
    int up, down, half;
    int in_lds;              // the table is staged in LDS (row stride 2 half + 1)
    long long taps_off;      // of row 0 in the table array
};

__host__ __device__ constexpr int rs_row_stride(int half) { return 2 * half + 1; }
// LDS bytes of a tile: the span (rounded up to 16 bytes), then the table if it is staged
__host__ __device__ constexpr long long rs_span_bytes(long long up, long long down, long long half) {
    return (rs_span(up, down, half) * (long long)sizeof(int) + 15) / 16 * 16;
}
__host__ __device__ constexpr long long rs_table_bytes(long long up, long long half) {
    return up * rs_row_stride((int)half) * (long long)sizeof(float);
}

// the channel sum of frame j of a file of n_in frames (0 outside it)
__device__ inline int rs_frame_sum(const int16_t* __restrict__ in, long long n_in, int C, bool pairs, long long j) {
    if (j < 0 || j >= n_in) return 0;
    if (pairs) {                                           // stereo at a 4-byte aligned address: one load
        const int v = ((const int*)in)[j];
        return (int)(short)(v & 0xffff) + (v >> 16);
    }
    int v = 0;
    for (int ch = 0; ch < C; ++ch) v += in[j * C + ch];
    return v;
}

__device__ inline int16_t rs_round(double acc, int C) {
    double y = rint(acc / (double)C);
    y = y < -32768.0 ? -32768.0 : (y > 32767.0 ? 32767.0 : y);
    return (int16_t)(int)y;
}

template <class Row>
__device__ inline double rs_dot(Row row, const int* __restrict__ sp, int n) {
    double acc = 0.0;
#pragma unroll 8
    for (int k = 0; k < n; ++k) acc = fma((double)row[k], (double)sp[k], acc);
    return acc;
}

__global__ __launch_bounds__(RS_TPB) void k_resample(
        const int16_t* __restrict__ in, const long long* __restrict__ in_off, const long long* __restrict__ out_off,
        const long long* __restrict__ tile_off /* [n_files + 1] each */, long long n_files,
        const int* __restrict__ channels, const int* __restrict__ conv_of /* [n_files] each */,
        const RsConv* __restrict__ convs, const float* __restrict__ taps, int16_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char rs_lds[];
    const int tid = threadIdx.x;
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const int C = channels[file];
    const RsConv cv = convs[conv_of[file]];
    const long long n_in = (in_off[file + 1] - in_off[file]) / C;
    const long long n_out = out_off[file + 1] - out_off[file];
    const long long n0 = ((long long)blockIdx.x - tile_off[file]) * RS_TILE;        // in the file
    const int cnt = (int)(n_out - n0 < RS_TILE ? n_out - n0 : RS_TILE);
    in += in_off[file];
    out += out_off[file] + n0;
    const bool pairs = C == 2 && ((unsigned long long)in & 3ull) == 0;
    if (cv.half == 0) {
        for (int r = tid; r < cnt; r += RS_TPB) out[r] = rs_round((double)rs_frame_sum(in, n_in, C, pairs, n0 + r), C);
        return;
    }
    const unsigned L = (unsigned)cv.up, M = (unsigned)cv.down;
    const int n_taps = 2 * cv.half;
    const long long at = n0 * (long long)M;
    const long long i0 = at / L;                              // input frame of the tile's first output
    const unsigned p0 = (unsigned)(at - i0 * L);              // and its phase
    const int span = (int)((p0 + (unsigned)(cnt - 1) * M) / L) + n_taps;      // <= rs_span(up, down, half)
    int* s = (int*)rs_lds;                                    // s[e]: frame i0 - half + 1 + e
    float* h = (float*)(rs_lds + rs_span_bytes(L, M, cv.half));
    const long long j0 = i0 - cv.half + 1;
    for (int e = tid; e < span; e += RS_TPB) s[e] = rs_frame_sum(in, n_in, C, pairs, j0 + e);
    const float* g = taps + cv.taps_off;
    const int stride = rs_row_stride(cv.half);
    if (cv.in_lds)
        for (int e = tid; e < (int)L * n_taps; e += RS_TPB) {
            const int row = e / n_taps;
            h[row * stride + (e - row * n_taps)] = g[e];
        }
    __syncthreads();
    for (int r = tid; r < cnt; r += RS_TPB) {
        const unsigned t = p0 + (unsigned)r * M;
        const unsigned q = t / L, ph = t - q * L;
        const double acc = cv.in_lds ? rs_dot((const float*)(h + ph * stride), s + q, n_taps)
                                     : rs_dot(g + (long long)ph * n_taps, s + q, n_taps);
        out[r] = rs_round(acc, C);
    }
}

}  // namespace spkd
