// The frame around the three batch decoders (k_vad_viterbi / k_vad_backtrack, k_mindur_viterbi /
// k_mindur_backtrack, k_fb_posterior): every rule they share.  The chain inside one sequence is serial
// and the sequences are independent, so a sequence is a group of lanes and every sequence of the
// batch runs in the same launch.  k_vad_viterbi and the two backtracks are built from these helpers;
// k_fb_posterior takes its score loads from here and k_mindur_viterbi spells the same rules out, because
// built from the helpers they compile to another schedule that measures slower (their headers say where;
// profiles/decoder_frame.json has the runs).
//
//   the group    G lanes (the power of two >= the word count, 1 .. LG_MAX) per sequence, one lane per
//                word, 64 / G sequences per wave, one wave per workgroup; lanes j >= the word count
//                idle along.  The wave runs to its longest sequence (Tmax), so every lane reaches every
//                ballot and shuffle; what a lane does behind its own T is masked by the kernels.
//   the scores   not on the dependent chain: a lane holds its word's score of TILE frames in registers
//                and loads the next tile while the chain runs over this one (the S floats of a frame
//                are contiguous, so the lanes of a group, and the groups' lines, share cache lines).
//                A frame outside [0, T) and an idle lane read 0.
//   cleaning     o_t(k): NaN counts as -inf; a frame whose words are all -inf counts as 0 for every
//                word.  (k_fb_posterior needs the group's maximum anyway and states it through that:
//                fb_emit.)
//   the best     the maximum over the group with the index it came from, as the host's scan `best =
//                v[0]; for i = 1..: if (v[i] > best) ...` leaves them: the lowest index among equals.
//                NAN0 restates the scan for NaNs: one at an index > 0 never beats anything (it counts
//                as -inf, and -inf at a higher index never wins), one at index 0 stays whatever follows.
//   the records  back-pointers, one record of type Rec per frame, a tile's records packed into 32-bit
//                words in the registers of the group's first lane and stored as 16-byte vectors.  A
//                sequence's records start at a multiple of TILE, so a tile's store never crosses into
//                the next sequence; records behind T - 1 are stored and never read.
//   the walk     one lane per sequence walks the records from the last frame, a tile at a time with
//                the tile below fetched ahead.  COUNT pass: the number of tokens; WRITE pass, after the
//                host has placed every sequence at its exact offset: first frame and word of every
//                token, written from the back so that they come out in order.  A write is checked
//                against the sequence's count.
//   the ending   the best of the last frame's d over the group: the final word, and the score (-inf
//                for a sequence without frames), written by the group's first lane.
//
// Everything is forced inline and every array index is a constant once the callers' loops are
// unrolled: the tiles stay in registers.  No helper adds or multiplies a floating-point value, so
// none depends on the caller's `fp contract`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"

namespace spkd {

constexpr int LG_MAX = 16;           // lanes of the widest group: states, words (GM_MAX_S)

template <int G>
struct LaneGroup {
    int lane, j, sh;                 // the lane, its word, the group's first lane
    long long f, row0, T, Tmax;      // the sequence, its first frame and frame count; the wave's longest
    bool has;                        // f is a sequence of the call
};

template <int G>
__device__ __forceinline__ LaneGroup<G> lg_setup(const long long* __restrict__ frame_off, long long n_seq) {
    LaneGroup<G> g;
    g.lane = threadIdx.x, g.j = g.lane % G, g.sh = g.lane - g.j;
    g.f = (long long)blockIdx.x * (WAVE / G) + g.lane / G;
    g.has = g.f < n_seq;
    g.row0 = g.has ? frame_off[g.f] : 0;
    g.T = g.has ? frame_off[g.f + 1] - g.row0 : 0;
    long long Tmax = g.T;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const long long o = __shfl_xor(Tmax, m);
        Tmax = o > Tmax ? o : Tmax;
    }
    g.Tmax = Tmax;
    return g;
}

// the group's G bits of a ballot
template <int G>
constexpr unsigned LG_MASK = (1u << G) - 1u;

template <int G>
__device__ __forceinline__ unsigned lg_bits(unsigned long long ballot, int sh) {
    return (unsigned)(ballot >> sh) & LG_MASK<G>;
}

// The score of frame t at sc (the sequence's frame 0, the lane's column).  Per frame, the loop over
// the tile stays with the kernel: filling a tile through a reference costs k_vad_viterbi and
// k_mindur_viterbi<1, true> a dozen registers and with them the second wave of a SIMD.
__device__ __forceinline__ float lg_score(const float* __restrict__ sc, int S, bool word, long long t, long long T) {
    return (word && t >= 0 && t < T) ? sc[t * S] : 0.0f;
}

// the tile fetched ahead becomes the current one
template <class V, int N>
__device__ __forceinline__ void lg_take(V (&cur)[N], const V (&nxt)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) cur[k] = nxt[k];
}

template <int G>
__device__ __forceinline__ double lg_clean(float s, bool word, int sh) {
    double o = s != s ? -INFINITY : (double)s;                               // NaN counts as -inf
    if (lg_bits<G>(__ballot(!word || o == -INFINITY), sh) == LG_MASK<G>) o = 0.0;   // every word -inf: 0 for every word
    return o;
}

template <int G, bool NAN0>
__device__ __forceinline__ double lg_best(double v, bool word, int j, int& idx) {
    if (!word || (NAN0 && j > 0 && v != v)) v = -INFINITY;
    idx = j;
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const double vo = __shfl_xor(v, m);
        const int io = __shfl_xor(idx, m);
        if (vo > v || (vo == v && io < idx) || (NAN0 && vo != vo)) { v = vo; idx = io; }
    }
    return v;
}

template <class Rec, int TILE>
struct LgRecords {                   // a tile's records
    static constexpr int BITS = 8 * (int)sizeof(Rec), PER = 32 / BITS, NPK = TILE / PER;
    static_assert(NPK % 4 == 0, "a tile's records are whole 16-byte vectors");
    unsigned pk[NPK];

    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < NPK; ++q) pk[q] = 0u;
    }
    __device__ __forceinline__ void put(int k, unsigned rec) { pk[k / PER] |= rec << (BITS * (k % PER)); }
    __device__ __forceinline__ unsigned get(int k) const { return (pk[k / PER] >> (BITS * (k % PER))) & (unsigned)(Rec)~(Rec)0; }
    // at: the sequence's first record; t0 a multiple of TILE
    __device__ __forceinline__ void store(Rec* at, long long t0) const {
        uint4* dst = reinterpret_cast<uint4*>(at + t0);
#pragma unroll
        for (int q = 0; q < NPK / 4; ++q) dst[q] = make_uint4(pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]);
    }
    __device__ __forceinline__ void fetch(const Rec* at, long long t0) {
        const uint4* src = reinterpret_cast<const uint4*>(at + t0);
#pragma unroll
        for (int q = 0; q < NPK / 4; ++q) {
            const uint4 v = src[q];
            pk[4 * q] = v.x, pk[4 * q + 1] = v.y, pk[4 * q + 2] = v.z, pk[4 * q + 3] = v.w;
        }
    }
};

template <bool WRITE>
struct LgWalk {                      // a backtrack's lane: its sequence, where the path is, the tokens so far
    long long f, T, cap, end, n;
    int j;
    long long *tok_frame;
    int* tok_word;

    // false: no sequence for this lane
    __device__ __forceinline__ bool begin(const long long* __restrict__ frame_off, long long n_seq,
                                          const int* __restrict__ final_word, const long long* __restrict__ tok_off,
                                          long long* __restrict__ frames, int* __restrict__ words) {
        f = (long long)blockIdx.x * WAVE + threadIdx.x;
        if (f >= n_seq) return false;
        T = frame_off[f + 1] - frame_off[f];
        cap = WRITE ? tok_off[f + 1] - tok_off[f] : 0, end = WRITE ? tok_off[f + 1] : 0;
        j = final_word[f];
        n = 0, tok_frame = frames, tok_word = words;
        return true;
    }
    // a token of word j from frame `first` on
    __device__ __forceinline__ void emit(long long first) {
        if (WRITE && n < cap) {
            tok_frame[end - 1 - n] = first;
            tok_word[end - 1 - n] = j;
        }
        ++n;
    }
    __device__ __forceinline__ void finish(long long* __restrict__ count) const {
        if (!WRITE) count[f] = n;
    }
};

// d_last: the lane's d of frame T - 1
template <int G, bool NAN0>
__device__ __forceinline__ void lg_ending(const LaneGroup<G>& g, bool word, double d_last, int* __restrict__ final_word,
                                          double* __restrict__ final_score) {
    int bj;
    const double v = lg_best<G, NAN0>(d_last, word, g.j, bj);                // max_j d_{T-1}(j), the lowest j among equals
    if (g.has && g.j == 0) {
        final_word[g.f] = bj;
        final_score[g.f] = g.T > 0 ? v : -INFINITY;
    }
}

}  // namespace spkd
