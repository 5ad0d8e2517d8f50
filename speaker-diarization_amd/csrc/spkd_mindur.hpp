// Viterbi over a loop of one-state speakers with a minimum duration (spkd_mindur_viterbi_batch): no
// stretch of a decoded path is shorter than D frames -- the one exception is a sequence of fewer than
// D frames, which is a single stretch.  A switch penalty alone (spkd_vad_viterbi_batch) cannot promise
// that: on frames that are correlated in time a burst of a few dozen frames beats any penalty that
// still lets real changes through.  PARITY: no reference counterpart (the reference stops at
// clustering); tests/reseg_mindur_numpy.py restates the recurrence and checks it against a brute-force
// decoder over the expanded state space (every word a left-to-right chain of D tied states).
//
// The recurrence, in fp64, in this order of operations (include/spkd.h (8) states it as the contract):
//   o_t(k)   the cleaned score: NaN counts as -inf; a frame whose words are all -inf counts as 0 for
//            every word.
//   P_t(k)   the sum of the finite o_u(k), u <= t, added in frame order from 0.0; C_t(k) the number of
//            -inf among them; P_-1 = C_-1 = 0.
//   w_t(k)   -inf if C_t(k) - C_{t-D}(k) > 0, else P_t(k) - P_{t-D}(k): the last D frames in word k.
//   d_t(k)   -inf for t < D - 1;  d_{D-1}(k) = (-penalty) + w_{D-1}(k);  for t >= D, with g, b the
//            maximum and the lowest arg-max over k of d_{t-D}(k) (both -inf, word 0 while t - D < D - 1):
//            stay = d_{t-1}(k) + o_t(k), fresh = (g - penalty) + w_t(k), d_t(k) = stay if stay >= fresh,
//            else fresh with entered_t(k) set.  Staying wins ties.  No NaN arises: the P are finite.
//   end      k* the lowest arg-max of d_{T-1}(k), the score that value.  T < D: one token (0, k*), k*
//            the lowest k that maximises (C_{T-1}(k) > 0 ? -inf : P_{T-1}(k)), score (-penalty) + that.
//            T == 0: no token, score -inf.
//   path     from (T - 1, k*), at (t, j): t <= D - 1: token (0, j), done; entered_t(j): token
//            (t - D + 1, j), then j = b_{t-D}, t = t - D; otherwise t = t - 1.
// A sequence whose words all hold a -inf somewhere in every window has d = -inf throughout: it comes
// out as the one token (0, 0) with score -inf.
//
//   k_mindur_viterbi   : the lane-group frame of spkd_lanegroup.hpp (a group of lanes per sequence, a
//                        lane per word), spelt out here, with two score streams, each MD_TILE frames in registers
//                        with the next tile in flight: the leading frame t and the trailing frame
//                        t - D, the same load D frames back.  The trailing stream rebuilds P_{t-D}
//                        with the same additions in the same order, so it is bit-equal to the
//                        leading sum of D frames earlier and nothing per word is stored; of the
//                        counts only the difference C_t - C_{t-D} is kept.  What is stored per frame
//                        is g_t (8 bytes) and b_t (4 bytes), by lane 0 of the group, which is also
//                        the lane that reads g back D frames later and hands it to the group by
//                        shuffle: no lane ever reads what another lane wrote.  D >= 2 MD_TILE (FAR):
//                        g_{t-D} comes from the global scratch, a tile fetched one tile ahead --
//                        every frame of it was stored before the current tile began.  D < 2 MD_TILE
//                        (NEAR): from a ring of 2 MD_TILE entries per group in LDS.  Only d + o, one
//                        comparison and one select are on the dependent chain; the maximum over the
//                        group is needed D frames later.  The back-pointer record is the group's
//                        `entered` ballot, 2 bytes a frame.  A sequence's records, g and b start at a
//                        multiple of MD_TILE.
//   k_mindur_backtrack : the frame's walk, which jumps D frames where the path entered a word,
//                        reading b there, and fetches the tile it lands in when that is not the
//                        tile below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_lanegroup.hpp"

namespace spkd {

constexpr int MD_TILE = 32;          // frames per score / record tile (SPKD_MINDUR_TILE)
constexpr int MD_RING = 2 * MD_TILE; // entries of a group's LDS ring; D below it decodes NEAR

// k_mindur_viterbi states the frame's rules itself (the group, the loads, the cleaning, the best, the
// records), as spkd_lanegroup.hpp words them: built from the shared helpers the same arithmetic comes
// out in another schedule, and the FAR form measures 1.3 - 3.5 % slower, outside the spread of its
// runs (profiles/decoder_frame.json).  A change to a rule there is a change here.
// max over the group's v with the lowest index among equals (no NaN comes here)
template <int G>
__device__ inline void md_best(double& v, int& idx) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const double vo = __shfl_xor(v, m);
        const int io = __shfl_xor(idx, m);
        if (vo > v || (vo == v && io < idx)) { v = vo; idx = io; }
    }
}

template <int G, bool NEAR>
__global__ __launch_bounds__(WAVE) void k_mindur_viterbi(
        const float* __restrict__ scores /* [sum T][S] */, const long long* __restrict__ frame_off /* [n_seq + 1] */,
        const long long* __restrict__ rec_off /* [n_seq + 1], multiples of MD_TILE */, long long n_seq, int S, int W,
        double penalty, long long D, uint16_t* __restrict__ rec, double* gbuf /* stored and read back: no restrict */,
        int* __restrict__ bbuf, int* __restrict__ final_word /* [n_seq] */, double* __restrict__ final_score /* [n_seq] */) {
#pragma clang fp contract(off)
    constexpr int NPK = MD_TILE / 2;                     // 32-bit words of a tile's records
    constexpr unsigned long long GMASK = (1ull << G) - 1ull;
    __shared__ double ring[NEAR ? WAVE / G : 1][NEAR ? MD_RING : 1];
    const int lane = threadIdx.x, j = lane % G, sh = lane - j;
    const long long f = (long long)blockIdx.x * (WAVE / G) + lane / G;
    const bool has = f < n_seq, word = j < W, lead = has && j == 0;
    const long long T = has ? frame_off[f + 1] - frame_off[f] : 0;
    const long long ro = has ? rec_off[f] : 0;
    const float* sc = scores + (has ? frame_off[f] * S : 0) + (word ? j : 0);
    const double npen = -penalty;
    long long Tmax = T;                                  // the wave runs to its longest sequence
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const long long o = __shfl_xor(Tmax, m);
        Tmax = o > Tmax ? o : Tmax;
    }
    float cur[MD_TILE], nxt[MD_TILE], tcur[MD_TILE], tnxt[MD_TILE];
    double gcur[NEAR ? 1 : MD_TILE], gnxt[NEAR ? 1 : MD_TILE];
#pragma unroll
    for (int k = 0; k < MD_TILE; ++k) {
        cur[k] = (word && k < T) ? sc[(long long)k * S] : 0.0f;
        const long long u = k - D;                       // (D >= 1: u < k)
        tcur[k] = (word && u >= 0 && u < T) ? sc[u * S] : 0.0f;
        if (!NEAR) gcur[k] = -INFINITY;                  // (t < MD_TILE <= D: never used)
    }
    double d = -INFINITY, d_last = -INFINITY, p_lead = 0.0, p_trail = 0.0;
    int ninf_win = 0;                                    // C_t - C_{t-D}
    for (long long t0 = 0; t0 < Tmax; t0 += MD_TILE) {
#pragma unroll
        for (int k = 0; k < MD_TILE; ++k) {
            const long long t = t0 + MD_TILE + k, u = t - D;
            nxt[k] = (word && t < T) ? sc[t * S] : 0.0f;
            tnxt[k] = (word && u >= 0 && u < T) ? sc[u * S] : 0.0f;
            // FAR: u <= t0 + 2 MD_TILE - 1 - D < t0, stored before this tile began
            if (!NEAR) gnxt[k] = (lead && u >= 0 && u < T) ? gbuf[ro + u] : -INFINITY;
        }
        unsigned pk[NPK];
#pragma unroll
        for (int q = 0; q < NPK; ++q) pk[q] = 0u;
#pragma unroll
        for (int k = 0; k < MD_TILE; ++k) {
            const long long t = t0 + k, u = t - D;
            const float s = cur[k], st = tcur[k];
            double o = s != s ? -INFINITY : (double)s;                       // NaN counts as -inf
            double ot = st != st ? -INFINITY : (double)st;
            const unsigned long long ninf = __ballot(!word || o == -INFINITY);
            const unsigned long long ninft = __ballot(!word || ot == -INFINITY);
            if (((ninf >> sh) & GMASK) == GMASK) o = 0.0;                    // every word -inf: 0 for every word
            if (((ninft >> sh) & GMASK) == GMASK) ot = 0.0;
            if (o == -INFINITY) ++ninf_win; else p_lead = p_lead + o;
            if (u >= 0) {
                if (ot == -INFINITY) --ninf_win; else p_trail = p_trail + ot;
            }
            const double w = ninf_win > 0 ? -INFINITY : p_lead - p_trail;
            double g = -INFINITY;                                            // g_{t-D}, from the group's lane 0
            if (NEAR) {
                if (lead && u >= 0) g = ring[lane / G][u & (MD_RING - 1)];
            } else {
                g = gcur[k];
            }
            g = __shfl(g, sh);
            const double stay = d + o, fresh = (t == D - 1 ? npen : g - penalty) + w;
            const bool stays = stay >= fresh;
            d = t < D - 1 ? -INFINITY : (stays ? stay : fresh);
            const unsigned long long entered = __ballot(word && !stays && t >= D);
            if (t == T - 1) d_last = T < D ? npen + w : d;                   // (T < D: no trailing frame, w is the whole sum)
            double gt = word ? d : -INFINITY;                                // g_t, b_t: read again D frames on
            int bt = j;
            md_best<G>(gt, bt);
            if (lead && t < T) {
                if (NEAR) ring[lane / G][t & (MD_RING - 1)] = gt; else gbuf[ro + t] = gt;
                bbuf[ro + t] = bt;
            }
            pk[k / 2] |= (unsigned)((entered >> sh) & GMASK) << (16 * (k % 2));
        }
        if (lead && t0 < T) {                            // (frames behind T - 1 of the tile: never read)
            uint4* dst = reinterpret_cast<uint4*>(rec + ro + t0);
#pragma unroll
            for (int q = 0; q < NPK / 4; ++q) dst[q] = make_uint4(pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]);
        }
#pragma unroll
        for (int k = 0; k < MD_TILE; ++k) {
            cur[k] = nxt[k];
            tcur[k] = tnxt[k];
            if (!NEAR) gcur[k] = gnxt[k];
        }
    }
    double v = word ? d_last : -INFINITY;                // max_k d_{T-1}(k), the lowest k among equals
    int bj = j;
    md_best<G>(v, bj);
    if (lead) {
        final_word[f] = bj;
        final_score[f] = T > 0 ? v : -INFINITY;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(WAVE) void k_mindur_backtrack(
        const uint16_t* __restrict__ rec, const int* __restrict__ bbuf, const long long* __restrict__ frame_off,
        const long long* __restrict__ rec_off, long long n_seq, long long D, const int* __restrict__ final_word,
        long long* __restrict__ count /* [n_seq]: COUNT pass out */, const long long* __restrict__ tok_off /* [n_seq + 1] */,
        long long* __restrict__ tok_frame, int* __restrict__ tok_word) {
    LgWalk<WRITE> w;
    if (!w.begin(frame_off, n_seq, final_word, tok_off, tok_frame, tok_word)) return;
    const uint16_t* src = rec + rec_off[w.f];
    const int* bs = bbuf + rec_off[w.f];
    long long tc = w.T - 1;                              // tc: the frame the path is at
    LgRecords<uint16_t, MD_TILE> cur, nxt;
    long long t0 = tc >= 0 ? tc / MD_TILE * MD_TILE : 0;
    if (tc >= 0) cur.fetch(src, t0);
    while (tc >= 0) {
        if (t0 >= MD_TILE) nxt.fetch(src, t0 - MD_TILE);
#pragma unroll
        for (int k = MD_TILE - 1; k >= 0; --k) {
            const long long t = t0 + k;
            if (t != tc) continue;                       // (behind T - 1, or jumped over)
            const bool entered = (cur.get(k) >> w.j) & 1u;                   // (set only for t >= D)
            long long first = -1;
            if (t <= D - 1) { first = 0; tc = -1; }
            else if (entered) { first = t - D + 1; tc = t - D; }
            else tc = t - 1;
            if (first >= 0) {
                w.emit(first);
                if (first > 0) w.j = bs[t - D];
            }
        }
        if (tc < 0) break;
        const long long below = t0 - MD_TILE;
        t0 = tc / MD_TILE * MD_TILE;
        if (t0 == below) cur = nxt; else cur.fetch(src, t0);
    }
    w.finish(count);
}

}  // namespace spkd
