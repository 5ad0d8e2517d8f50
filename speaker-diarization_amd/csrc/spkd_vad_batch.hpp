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
//   k_vad_viterbi   : the lane-group frame of spkd_lanegroup.hpp (a group of lanes per file, a lane
//                     per word, the scores a tile of VB_TILE frames ahead of the chain) around the
//                     recurrence of include/spkd.h in fp64 sums and comparisons, in the header's
//                     order.  The max over d(i) + exit_i is the group's best with the host's scan
//                     restated for NaNs.  Back-pointers: per frame one record -- bit j: word j was
//                     entered, bits G..G+3: bi, the word left -- of 2 bytes (W <= 8) or 4 bytes
//                     (W > 8), at most W + 1 bytes; the group's flags come from one ballot.
//   k_vad_backtrack : the frame's walk: a token where the path enters a word, and at frame 0; the
//                     word left is the record's bi.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_lanegroup.hpp"

namespace spkd {

constexpr int VB_TILE = 32;          // frames per score / back-pointer tile (SPKD_VAD_TILE)
constexpr int VB_SHIFT_TPB = 256;

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
    double e[LG_MAX];
#pragma unroll
    for (int r = 0; r < LG_MAX; ++r) e[r] = r < S ? exp((double)in[base + r * T]) : 0.0;
    e[1] = e[1] * shift;
    double sum = e[0];
#pragma unroll
    for (int r = 1; r < LG_MAX; ++r)
        if (r < S) sum = sum + e[r];
#pragma unroll
    for (int r = 0; r < LG_MAX; ++r)
        if (r < S) out[base + r * T] = (float)log(e[r] / sum);
}

template <int G>
__global__ __launch_bounds__(WAVE) void k_vad_viterbi(
        const float* __restrict__ scores /* [sum T][S] */, const long long* __restrict__ frame_off /* [n_files + 1] */,
        const long long* __restrict__ back_off /* [n_files + 1], multiples of VB_TILE */, long long n_files, int S, int W,
        const int* __restrict__ word_state, const double* __restrict__ c_stay, const double* __restrict__ c_exit,
        const double* __restrict__ c_enter, typename VbRecord<G>::type* __restrict__ back,
        int* __restrict__ final_word /* [n_files] */, double* __restrict__ final_score /* [n_files] */) {
    const LaneGroup<G> g = lg_setup<G>(frame_off, n_files);
    const int j = g.j;
    const bool word = j < W;
    const long long T = g.T;
    const float* sc = scores + g.row0 * S + (word ? word_state[j] : 0);
    const double stay_c = word ? c_stay[j] : 0.0, exit_c = word ? c_exit[j] : 0.0, enter_c = word ? c_enter[j] : 0.0;
    float cur[VB_TILE], nxt[VB_TILE];
#pragma unroll
    for (int k = 0; k < VB_TILE; ++k) cur[k] = lg_score(sc, S, word, k, T);
    double d = 0.0, d_last = -INFINITY;
    for (long long t0 = 0; t0 < g.Tmax; t0 += VB_TILE) {
#pragma unroll
        for (int k = 0; k < VB_TILE; ++k) nxt[k] = lg_score(sc, S, word, t0 + VB_TILE + k, T);
        LgRecords<typename VbRecord<G>::type, VB_TILE> recs;
        recs.clear();
#pragma unroll
        for (int k = 0; k < VB_TILE; ++k) {
            const long long t = t0 + k;
            const double o = lg_clean<G>(cur[k], word, g.sh);
            int bi;
            const double v = lg_best<G, true>(d + exit_c, word, j, bi);
            const double stay = d + stay_c, sw = v + enter_c;
            const bool stays = stay >= sw, first = t == 0;
            d = (first ? enter_c : (stays ? stay : sw)) + o;
            if (t == T - 1) d_last = d;
            recs.put(k, lg_bits<G>(__ballot(word && !first && !stays), g.sh) | ((unsigned)bi << G));
        }
        if (j == 0 && t0 < T) recs.store(back + back_off[g.f], t0);
        lg_take(cur, nxt);
    }
    lg_ending<G, true>(g, word, d_last, final_word, final_score);
}

template <class Rec, bool WRITE>
__global__ __launch_bounds__(WAVE) void k_vad_backtrack(
        const Rec* __restrict__ back, const long long* __restrict__ frame_off, const long long* __restrict__ back_off,
        long long n_files, int gbits /* G of the decoding launch */, const int* __restrict__ final_word,
        long long* __restrict__ count /* [n_files]: COUNT pass out */, const long long* __restrict__ tok_off /* [n_files + 1] */,
        long long* __restrict__ tok_frame, int* __restrict__ tok_word) {
    LgWalk<WRITE> w;
    if (!w.begin(frame_off, n_files, final_word, tok_off, tok_frame, tok_word)) return;
    const Rec* src = back + back_off[w.f];
    LgRecords<Rec, VB_TILE> cur, nxt;
    long long t0 = w.T > 0 ? (w.T - 1) / VB_TILE * VB_TILE : -1;
    if (t0 >= 0) cur.fetch(src, t0);
    for (; t0 >= 0; t0 -= VB_TILE) {
        if (t0 >= VB_TILE) nxt.fetch(src, t0 - VB_TILE);
#pragma unroll
        for (int k = VB_TILE - 1; k >= 0; --k) {
            const long long t = t0 + k;
            if (t >= w.T) continue;
            const unsigned rec = cur.get(k);
            const bool entered = (rec >> w.j) & 1u;
            if (t == 0 || entered) w.emit(t);            // a token where the path enters a word, and at frame 0
            if (entered) w.j = (int)(rec >> gbits);
        }
        cur = nxt;
    }
    w.finish(count);
}

}  // namespace spkd
