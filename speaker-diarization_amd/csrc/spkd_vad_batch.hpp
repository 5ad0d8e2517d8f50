// Speech / non-speech decision for a whole batch of files (spkd_vad_shift_batch,
// spkd_vad_viterbi_batch): the border shift of generate_exp.py:177-186 and the exact Viterbi of
// spkd_vad_viterbi, over the concatenated score array [sum T][S] float32 of the batch.  The chain
// inside one file is serial; the files are independent, so a file is a group of lanes and every
// file runs in the same launch.
//
//   k_vad_shift     : one lane per column of a file's (S, T) view -- the reference reshapes the
//                     frame-major block of T*S floats to (S, -1), row r = flat [r T, (r + 1) T) --
//                     exp in fp64, row 1 times the shift, divided by the sum of the rows in row
//                     order, log, rounded to float32.  A lane reads its S values before it writes
//                     any, and nobody else touches them: the call may run in place.  Naive IEEE
//                     on purpose (underflow gives -inf, 0 / 0 NaN), no contraction into FMAs.
//   k_vad_viterbi   : a group of G lanes (G = the power of two >= W) per file, one lane per word,
//                     64 / G files per wave, one wave per workgroup.  The recurrence of
//                     include/spkd.h in fp64 sums and comparisons, in the header's order.  The max
//                     over d(i) + exit_i is a butterfly over the group that keeps the lowest index
//                     on ties and restates the host's scan for NaNs (a NaN at word 0 stays, a NaN
//                     elsewhere never beats anything).  The scores are not on the dependent
//                     chain: a lane loads its word's score of the next VB_TILE frames into
//                     registers while the chain runs over the current tile (the S floats of a
//                     frame are contiguous and the lanes of a group, and the groups' lines, share
//                     cache lines).  Back-pointers: per frame one record -- bit j: word j was
//                     entered, bits G..G+3: bi, the word left -- of 2 bytes (W <= 8) or 4 bytes
//                     (W > 8), at most W + 1 bytes; the group's flags come from one ballot, lane
//                     0 of the group keeps the tile's records in registers and stores them as
//                     16-byte vectors.  A file's records start at a multiple of VB_TILE, so a
//                     tile's store never crosses into the next file.
//   k_vad_backtrack : one lane per file walks the records from the last frame, a tile (fetched one
//                     tile ahead) at a time.  COUNT pass: the number of tokens; WRITE pass, after
//                     the host has placed every file at its exact offset: first frame and word of
//                     every word the path enters, written from the back so that they come out in
//                     order.  A write is checked against the file's count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"

namespace spkd {

constexpr int VB_TILE = 32;          // frames per score / back-pointer tile (SPKD_VAD_TILE)
constexpr int VB_SHIFT_TPB = 256;
constexpr int VB_MAX = 16;           // states, words (GM_MAX_S)

template <int G> struct VbRecord { typedef uint16_t type; };
template <> struct VbRecord<16> { typedef uint32_t type; };

__global__ __launch_bounds__(VB_SHIFT_TPB) void k_vad_shift(
        const float* in /* [sum T][S]; may be out */, const long long* __restrict__ frame_off /* [n_files + 1] */,
        long long n_files, int S, double shift, float* out) {
#pragma clang fp contract(off)
    const long long g = (long long)blockIdx.x * VB_SHIFT_TPB + threadIdx.x;
    if (g >= frame_off[n_files]) return;
    long long lo = 0, hi = n_files;                      // the file of column g: frame_off[lo] <= g < frame_off[lo + 1]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) / 2;
        if (frame_off[mid] <= g) lo = mid; else hi = mid;
    }
    const long long T = frame_off[lo + 1] - frame_off[lo], i = g - frame_off[lo];
    const long long base = frame_off[lo] * S + i;
    double e[VB_MAX];
#pragma unroll
    for (int r = 0; r < VB_MAX; ++r) e[r] = r < S ? exp((double)in[base + r * T]) : 0.0;
    e[1] = e[1] * shift;
    double sum = e[0];
#pragma unroll
    for (int r = 1; r < VB_MAX; ++r)
        if (r < S) sum = sum + e[r];
#pragma unroll
    for (int r = 0; r < VB_MAX; ++r)
        if (r < S) out[base + r * T] = (float)log(e[r] / sum);
}

// max over the group's v with the index it came from, as the host's scan `best = v[0]; for i = 1..:
// if (v[i] > best) ...` leaves them: the lowest index among equals; the caller has replaced a NaN
// at an index > 0 by -inf (the scan never takes it, and -inf at a higher index never wins), a NaN
// at index 0 is what the scan keeps whatever follows.
template <int G>
__device__ inline void vb_best(double& v, int& idx) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const double vo = __shfl_xor(v, m);
        const int io = __shfl_xor(idx, m);
        if (vo > v || (vo == v && io < idx) || vo != vo) { v = vo; idx = io; }
    }
}

template <int G>
__global__ __launch_bounds__(WAVE) void k_vad_viterbi(
        const float* __restrict__ scores /* [sum T][S] */, const long long* __restrict__ frame_off /* [n_files + 1] */,
        const long long* __restrict__ back_off /* [n_files + 1], multiples of VB_TILE */, long long n_files, int S, int W,
        const int* __restrict__ word_state, const double* __restrict__ c_stay, const double* __restrict__ c_exit,
        const double* __restrict__ c_enter, typename VbRecord<G>::type* __restrict__ back,
        int* __restrict__ final_word /* [n_files] */, double* __restrict__ final_score /* [n_files] */) {
    typedef typename VbRecord<G>::type Rec;
    constexpr int PER = 4 / (int)sizeof(Rec);            // records per 32-bit word
    constexpr int NPK = VB_TILE / PER;
    constexpr unsigned long long GMASK = (1ull << G) - 1ull;
    const int lane = threadIdx.x, j = lane % G, sh = lane - j;
    const long long f = (long long)blockIdx.x * (WAVE / G) + lane / G;
    const bool has = f < n_files, word = j < W;
    const long long T = has ? frame_off[f + 1] - frame_off[f] : 0;
    const float* sc = scores + (has ? frame_off[f] * S : 0) + (word ? word_state[j] : 0);
    const double stay_c = word ? c_stay[j] : 0.0, exit_c = word ? c_exit[j] : 0.0, enter_c = word ? c_enter[j] : 0.0;
    long long Tmax = T;                                  // the wave runs to its longest file
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const long long o = __shfl_xor(Tmax, m);
        Tmax = o > Tmax ? o : Tmax;
    }
    float cur[VB_TILE], nxt[VB_TILE];
#pragma unroll
    for (int k = 0; k < VB_TILE; ++k) cur[k] = (word && k < T) ? sc[(long long)k * S] : 0.0f;
    double d = 0.0, d_last = -INFINITY;
    for (long long t0 = 0; t0 < Tmax; t0 += VB_TILE) {
#pragma unroll
        for (int k = 0; k < VB_TILE; ++k) {
            const long long t = t0 + VB_TILE + k;
            nxt[k] = (word && t < T) ? sc[t * S] : 0.0f;
        }
        unsigned pk[NPK];
#pragma unroll
        for (int q = 0; q < NPK; ++q) pk[q] = 0u;
#pragma unroll
        for (int k = 0; k < VB_TILE; ++k) {
            const long long t = t0 + k;
            const float s = cur[k];
            double o = s != s ? -INFINITY : (double)s;                       // NaN counts as -inf
            const unsigned long long ninf = __ballot(!word || o == -INFINITY);
            if (((ninf >> sh) & GMASK) == GMASK) o = 0.0;                    // every word -inf: 0 for every word
            double v = d + exit_c;
            if (!word || (j > 0 && v != v)) v = -INFINITY;
            int bi = j;
            vb_best<G>(v, bi);
            const double stay = d + stay_c, sw = v + enter_c;
            const bool stays = stay >= sw, first = t == 0;
            d = (first ? enter_c : (stays ? stay : sw)) + o;
            if (t == T - 1) d_last = d;
            const unsigned long long entered = __ballot(word && !first && !stays);
            const unsigned rec = (unsigned)((entered >> sh) & GMASK) | ((unsigned)bi << G);
            pk[k / PER] |= rec << (8 * (int)sizeof(Rec) * (k % PER));
        }
        if (j == 0 && t0 < T) {                          // (frames behind T - 1 of the tile: never read)
            uint4* dst = reinterpret_cast<uint4*>(back + back_off[f] + t0);
#pragma unroll
            for (int q = 0; q < NPK / 4; ++q) dst[q] = make_uint4(pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]);
        }
#pragma unroll
        for (int k = 0; k < VB_TILE; ++k) cur[k] = nxt[k];
    }
    double v = d_last;                                   // max_j d_{T-1}(j), the lowest j among equals
    if (!word || (j > 0 && v != v)) v = -INFINITY;
    int bj = j;
    vb_best<G>(v, bj);
    if (has && j == 0) {
        final_word[f] = bj;
        final_score[f] = T > 0 ? v : -INFINITY;
    }
}

template <class Rec, bool WRITE>
__global__ __launch_bounds__(WAVE) void k_vad_backtrack(
        const Rec* __restrict__ back, const long long* __restrict__ frame_off, const long long* __restrict__ back_off,
        long long n_files, int gbits /* G of the decoding launch */, const int* __restrict__ final_word,
        long long* __restrict__ count /* [n_files]: COUNT pass out */, const long long* __restrict__ tok_off /* [n_files + 1] */,
        long long* __restrict__ tok_frame, int* __restrict__ tok_word) {
    constexpr int PER = 4 / (int)sizeof(Rec);
    constexpr int NV = VB_TILE / PER / 4;                // 16-byte vectors per tile
    const long long f = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (f >= n_files) return;
    const long long T = frame_off[f + 1] - frame_off[f];
    const long long cap = WRITE ? tok_off[f + 1] - tok_off[f] : 0, end = WRITE ? tok_off[f + 1] : 0;
    const uint4* src = reinterpret_cast<const uint4*>(back + back_off[f]);
    int j = final_word[f];
    long long n = 0;
    uint4 cur[NV], nxt[NV];
    long long t0 = T > 0 ? (T - 1) / VB_TILE * VB_TILE : -1;
    if (t0 >= 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) cur[q] = src[t0 / VB_TILE * NV + q];
    }
    for (; t0 >= 0; t0 -= VB_TILE) {
        if (t0 >= VB_TILE) {
#pragma unroll
            for (int q = 0; q < NV; ++q) nxt[q] = src[(t0 / VB_TILE - 1) * NV + q];
        }
#pragma unroll
        for (int k = VB_TILE - 1; k >= 0; --k) {
            const long long t = t0 + k;
            if (t >= T) continue;
            const uint4 v4 = cur[k / PER / 4];
            const int w = (k / PER) % 4;
            const unsigned word32 = w == 0 ? v4.x : w == 1 ? v4.y : w == 2 ? v4.z : v4.w;
            const unsigned rec = (word32 >> (8 * (int)sizeof(Rec) * (k % PER))) & (unsigned)(Rec)~(Rec)0;
            const bool entered = (rec >> j) & 1u;
            if (t == 0 || entered) {                     // a token where the path enters a word, and at frame 0
                if (WRITE && n < cap) {
                    tok_frame[end - 1 - n] = t;
                    tok_word[end - 1 - n] = j;
                }
                ++n;
            }
            if (entered) j = (int)(rec >> gbits);
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) cur[q] = nxt[q];
    }
    if (!WRITE) count[f] = n;
}

}  // namespace spkd
