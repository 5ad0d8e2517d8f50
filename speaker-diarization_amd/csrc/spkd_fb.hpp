// Speaker posteriors of a batch of turns (spkd_fb_posterior_batch): the forward-backward pass over the
// speaker loop the decoders search (stay 0, switch -penalty) on the scores they decode.  Per sequence:
// the posterior probability gamma_t(k) of every word at every frame, per decoded token the mean
// posterior of its word (the confidence), and the log-evidence of the sequence.  The decoded path is
// the mode of this distribution; the confidence says how much of the mass sits near it.
// PARITY: no reference counterpart (the reference stops at clustering); tests/reseg_fb_numpy.py restates
// the recursion and checks it against an enumeration of all paths.
//
// The recursion, in fp64 (include/spkd.h (8) states it as the contract; it fixes values, not the
// order of the operations), n the sequence's word count, k < n:
//   o_t(k)   the cleaned score (spkd_lanegroup.hpp, over the sequence's n words).  m_t = max_k o_t(k),
//            b_t(k) = exp(scale (o_t(k) - m_t)).
//   q, r     q = exp(-scale penalty), r = 1 - q: a step keeps its word with weight r + q = 1 and
//            reaches any other with weight q.
//   forward  u_0 = b_0, u_t(k) = b_t(k) (r a_{t-1}(k) + q), s_t = sum_k u_t(k), a_t = u_t / s_t,
//            logz = -scale penalty + sum_t (scale m_t + ln s_t).
//   backward beta_{T-1} = 1, h(k) = b_{t+1}(k) beta_{t+1}(k), H = sum_k h(k), w(k) = r h(k) + q H,
//            beta_t = w / sum_k w(k).
//   gamma    gamma_t(k) = a_t(k) beta_t(k) / sum_j a_t(j) beta_t(j).
//
//   k_fb_posterior : the lane-group frame of spkd_lanegroup.hpp -- a group of lanes (the power of two >=
//                    n_cols) per sequence, a lane per word, the scores a tile of FB_TILE frames in
//                    registers with the next tile in flight, in the backward sweep the tile below.  One
//                    launch, two sweeps by the same lanes.  Forward: the a recursion and logz; stored
//                    is only the a that enters each tile, in fp64 (a forward value that would flush to 0
//                    in float32 can belong to the word the backward pass favours): 8 G bytes a tile.  A
//                    lane reads back only what it stored itself.  Backward, tile by tile from the end,
//                    the tile below fetched ahead: the tile's b once into registers, its a again from
//                    the stored one, then beta backwards and gamma.  sum_k w(k) is H (r + n q), so one
//                    sum over the group and one reciprocal are on the dependent chain of each sweep;
//                    the exps, logs and the sum of gamma are off it.  The lane of a token's word adds
//                    its gamma (compensated, as logz is: the sums run over thousands of frames) and
//                    writes sum / length when t passes the token's first frame; the sequence's tokens
//                    are walked backwards, the next one fetched ahead.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_lanegroup.hpp"

namespace spkd {

constexpr int FB_TILE = 32;          // frames per score tile and per stored forward vector (SPKD_FB_TILE)

template <int G>
__device__ inline double fb_sum(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <int G>
__device__ inline double fb_max(double v) {
#pragma unroll
    for (int m = 1; m < G; m <<= 1) {
        const double o = __shfl_xor(v, m);
        v = o > v ? o : v;
    }
    return v;
}

// sum += x, compensated (Kahan): c carries what the additions lost
__device__ inline void fb_add(double& sum, double& c, double x) {
    const double y = x - c, t = sum + y;
    c = (t - sum) - y;
    sum = t;
}

// b_t(k) and m_t from the lane's raw score: the cleaning of spkd_lanegroup.hpp inside, through the
// group's maximum, which is needed anyway
template <int G>
__device__ inline double fb_emit(float s, bool word, double scale, double& m) {
    double o = (!word || s != s) ? -INFINITY : (double)s;                    // NaN counts as -inf
    m = fb_max<G>(o);
    if (m == -INFINITY) {                                                    // every word -inf: 0 for every word
        o = word ? 0.0 : o;
        m = 0.0;
    }
    return word ? exp(scale * (o - m)) : 0.0;
}

template <int G>
__global__ __launch_bounds__(WAVE) void k_fb_posterior(
        const float* __restrict__ scores /* [sum T][S] */, const long long* __restrict__ frame_off /* [n_seq + 1] */,
        const long long* __restrict__ tile_off /* [n_seq + 1], in tiles */, const int* __restrict__ seq_n /* [n_seq] or null */,
        long long n_seq, int S, double penalty, double scale, const long long* __restrict__ tok_off /* [n_seq + 1] or null */,
        const long long* __restrict__ tok_frame, const int* __restrict__ tok_word,
        double* fwd /* [tiles][G]: stored and read back, no restrict */, float* __restrict__ post /* [sum T][S] or null */,
        double* __restrict__ conf /* [n_tok] */, double* __restrict__ logz /* [n_seq] */) {
#pragma clang fp contract(off)
    // The group as lg_setup states it, the tile hand-over as lg_take and the last tile's load as lg_score,
    // spelt out: through those helpers the compiler schedules this kernel's sweeps differently and it
    // measures slower than the spread of its runs (profiles/decoder_frame.json).
    const int lane = threadIdx.x, j = lane % G;
    const long long f = (long long)blockIdx.x * (WAVE / G) + lane / G;
    const bool has = f < n_seq;
    const int n = has ? (seq_n ? seq_n[f] : S) : 1;
    const bool word = j < n, col = has && j < S;
    const long long T = has ? frame_off[f + 1] - frame_off[f] : 0;
    const long long row0 = has ? frame_off[f] : 0;
    const float* sc = scores + row0 * S + (word ? j : 0);
    double* ck = fwd + (has ? tile_off[f] : 0) * G + j;
    const double q = exp(-(scale * penalty)), r = 1.0 - q, rcw = 1.0 / (r + (double)n * q);
    long long Tmax = T;                                  // the wave runs to its longest sequence
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const long long o = __shfl_xor(Tmax, m);
        Tmax = o > Tmax ? o : Tmax;
    }
    float cur[FB_TILE], nxt[FB_TILE];

    // ---- forward: a, logz, the a that enters each tile
#pragma unroll
    for (int k = 0; k < FB_TILE; ++k) cur[k] = lg_score(sc, S, word, k, T);
    double a = 0.0, lz = 0.0, lz_c = 0.0;
    for (long long t0 = 0; t0 < Tmax; t0 += FB_TILE) {
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) nxt[k] = lg_score(sc, S, word, t0 + FB_TILE + k, T);
        if (t0 < T) ck[t0 / FB_TILE * G] = a;
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) {
            const long long t = t0 + k;
            double m;
            const double b = fb_emit<G>(cur[k], word, scale, m);
            const double u = t == 0 ? b : b * (r * a + q);
            const double s = fb_sum<G>(u);
            if (t < T) {
                a = u * (1.0 / s);
                fb_add(lz, lz_c, scale * m + log(s));
            }
        }
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) cur[k] = nxt[k];
    }
    if (has && j == 0) logz[f] = T > 0 ? lz - scale * penalty : -INFINITY;

    // ---- backward, tile by tile from the end: b and a of the tile, beta, gamma, the tokens
    long long ti = -1, tfirst = 0, tend = T, nfirst = 0; // the running token, its frames [tfirst, tend); the one before it
    int tw = -1, nw = -1;
    if (has && tok_off && tok_off[f + 1] > tok_off[f]) {
        ti = tok_off[f + 1] - 1;
        tfirst = tok_frame[ti];
        tw = tok_word[ti];
        if (ti > tok_off[f]) { nfirst = tok_frame[ti - 1]; nw = tok_word[ti - 1]; }
    }
    const long long tlo = has && tok_off ? tok_off[f] : 0;
    double acc = 0.0, acc_c = 0.0, h = 0.0;              // h: b_{t+1} beta_{t+1}
    long long t0 = Tmax > 0 ? (Tmax - 1) / FB_TILE * FB_TILE : -1;
    if (t0 >= 0) {
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) cur[k] = (word && t0 + k < T) ? sc[(t0 + k) * S] : 0.0f;
    }
    for (; t0 >= 0; t0 -= FB_TILE) {
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) nxt[k] = lg_score(sc, S, word, t0 - FB_TILE + k, T);
        double bt[FB_TILE], at[FB_TILE];
        double av = t0 < T ? ck[t0 / FB_TILE * G] : 0.0;
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) {
            const long long t = t0 + k;
            double m;
            bt[k] = fb_emit<G>(cur[k], word, scale, m);
            const double u = t == 0 ? bt[k] : bt[k] * (r * av + q);
            const double s = fb_sum<G>(u);
            av = u * (1.0 / s);
            at[k] = av;
        }
#pragma unroll
        for (int k = FB_TILE - 1; k >= 0; --k) {
            const long long t = t0 + k;
            const double H = fb_sum<G>(h);
            double beta = word ? (r * h + q * H) * ((1.0 / H) * rcw) : 0.0;
            if (t == T - 1) beta = 1.0;
            const double g = word ? at[k] * beta : 0.0;
            const double gs = fb_sum<G>(g);
            const double gamma = word ? g / gs : 0.0;
            if (t < T) {
                h = bt[k] * beta;
                if (post && col) post[(row0 + t) * S + j] = (float)gamma;
                if (ti >= 0) {
                    if (j == tw) fb_add(acc, acc_c, gamma);
                    if (t == tfirst) {
                        if (j == tw) conf[ti] = acc / (double)(tend - tfirst);
                        acc = 0.0;
                        acc_c = 0.0;
                        tend = tfirst;
                        tfirst = nfirst;
                        tw = nw;
                        --ti;
                        if (ti < tlo) ti = -1;
                        else if (ti > tlo) { nfirst = tok_frame[ti - 1]; nw = tok_word[ti - 1]; }
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < FB_TILE; ++k) cur[k] = nxt[k];
    }
}

}  // namespace spkd
