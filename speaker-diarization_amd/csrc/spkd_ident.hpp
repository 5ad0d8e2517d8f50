// Identification of speaker records (spkd_ubm_stats.hpp) against a gallery of enrolled records by
// cross-likelihood ratio under MAP-adapted means (spkd_clr_identify), and the ordered sums of records
// that build a cluster's record and fold it into its identity (spkd_bw_accumulate).
// PARITY: no reference counterpart -- the reference keeps nothing from one run to the next
// (spk-clustering.py:289 is a TODO for more than one wav); tests/gallery_numpy.py restates the scores,
// the assignment and the sums in numpy.
//
// The score of probe s against identity g is spkd_clr.hpp's CLR of the two records: T and N of either
// side by clr_derive, the pair by clr_pair in its lane order (16 lanes, stride-16 terms, butterfly), so
// a pair's bits are those k_clr_matrix gives for the same two records.
//
//   k_ident_derive : a wave per record: its T and N (the gallery's once per call).
//   k_ident_scores : a workgroup per tile of ID_ROWS probe rows and ID_COLS gallery columns.  R, T and N
//                    of the rows wait in LDS; every 16-lane group strides over the columns, so a gallery
//                    record comes from memory once per row tile, coalesced; the tile's other rows find it
//                    in the vector cache.
//   k_ident_assign : ONE workgroup per group of probes (those that must get distinct identities).  Per
//                    row the best free column waits in LDS; a step is an arg-max over those (the first
//                    in row-major order on a tie), the pair assigned while its score is above the
//                    threshold, and a new scan of the rows whose best column was just taken, a wave a
//                    row -- k_clr_chain's idiom.  12 bytes a row and one bit a column.
//   k_bw_accumulate: a workgroup per set, a lane per element, plain additions in member order.
// No atomics on values; the bits depend neither on the run nor on the tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_clr.hpp"
#include "spkd_device.hpp"

namespace spkd {

constexpr int ID_MAX_G = 16384;       // identities of one call (SPKD_GALLERY_MAX_N): one bit each in k_ident_assign's LDS
constexpr int ID_ROWS = 4;            // k_ident_scores: probe rows of a tile
constexpr int ID_TPB = 256;           // k_ident_scores: 16 groups of CL_GROUP lanes
constexpr int ID_COLS = 256;          // k_ident_scores: gallery columns of a tile, 16 a group
constexpr int ID_MAX_E = GT_MAX_COMP * BW_COMP;
constexpr int ID_ACC_TPB = 320;       // k_bw_accumulate: a lane per element of a record
constexpr unsigned char ID_OPEN = 1, ID_RESCAN = 2;
static_assert(ID_ACC_TPB >= ID_MAX_E && ID_ACC_TPB % WAVE == 0, "a lane per element");
static_assert(ID_MAX_G % 32 == 0 && ID_TPB % CL_GROUP == 0 && ID_COLS % (ID_TPB / CL_GROUP) == 0, "tiles");

__global__ __launch_bounds__(WAVE) void k_ident_derive(const double* __restrict__ bw, const double* __restrict__ ubm,
                                                       int K, double r, double* __restrict__ T, double* __restrict__ Nn) {
    const long long s = blockIdx.x;
    const int E = K * BW_COMP;
    clr_derive(bw + s * E, ubm, K, r, T + s * E, Nn + s, threadIdx.x, WAVE);
}

// score[s][g] of the S probes against the G identities; NaN where either side is not ok
__global__ __launch_bounds__(ID_TPB) void k_ident_scores(
        const double* __restrict__ Rp, const double* __restrict__ Tp, const double* __restrict__ Np,
        const int* __restrict__ okp, int S, const double* __restrict__ Rg, const double* __restrict__ Tg,
        const double* __restrict__ Ng, const int* __restrict__ okg, int G, int K, double* __restrict__ score, int* err) {
    __shared__ double sR[ID_ROWS][ID_MAX_E], sT[ID_ROWS][ID_MAX_E];
    __shared__ double sN[ID_ROWS];
    __shared__ int sOk[ID_ROWS];
    const int E = K * BW_COMP;
    const int s0 = blockIdx.x * ID_ROWS;
    const int rows = S - s0 < ID_ROWS ? S - s0 : ID_ROWS;
    const int tid = threadIdx.x, sub = tid % CL_GROUP, grp = tid / CL_GROUP;
    for (int i = 0; i < rows; ++i)
        for (int e = tid; e < E; e += ID_TPB) {
            sR[i][e] = Rp[(long long)(s0 + i) * E + e];
            sT[i][e] = Tp[(long long)(s0 + i) * E + e];
        }
    if (tid < rows) {
        sN[tid] = Np[s0 + tid];
        sOk[tid] = okp[s0 + tid];
    }
    __syncthreads();
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int g0 = blockIdx.y * ID_COLS;
    const int g1 = G - g0 < ID_COLS ? G : g0 + ID_COLS;
    for (int g = g0 + grp; g < g1; g += ID_TPB / CL_GROUP) {
        const int good = okg[g];                                        // (uniform in the group)
        const double* __restrict__ rg = Rg + (long long)g * E;
        const double* __restrict__ tg = Tg + (long long)g * E;
        const double ng = Ng[g];
        for (int i = 0; i < rows; ++i) {
            double v = nan;
            if (good && sOk[i]) {                                       // (uniform in the group)
                v = clr_pair(sR[i], sT[i], sN[i], rg, tg, ng, E, sub);
                if (sub == 0 && !gt_finite(v)) atomicOr(err, ERR_NONFINITE);
            }
            if (sub == 0) score[(long long)(s0 + i) * G + g] = v;
        }
    }
}

// Over the columns of one row whose bit in `closed` is clear, by one wave: the highest value v1 at
// the lowest such column j1 (-1: no column), and v2, the highest among the columns other than j1
// (-inf: none).  The same in every lane.
__device__ inline void ident_row_scan(const double* __restrict__ row, const unsigned* closed, int G, int lane,
                                      double& v1, int& j1, double& v2) {
    v1 = v2 = -INFINITY;
    j1 = -1;
    for (int j = lane; j < G; j += WAVE) {
        if ((closed[j >> 5] >> (j & 31)) & 1u) continue;
        const double v = row[j];
        if (j1 < 0 || v > v1) {
            if (j1 >= 0) v2 = v1;
            v1 = v;
            j1 = j;
        } else if (v > v2) {
            v2 = v;
        }
    }
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const double o1 = __shfl_xor(v1, m), o2 = __shfl_xor(v2, m);
        const int oj = __shfl_xor(j1, m);
        if (oj < 0) continue;                                           // (the other half saw no column)
        if (j1 < 0 || o1 > v1 || (o1 == v1 && oj < j1)) {
            const double mine = j1 >= 0 ? v1 : -INFINITY;
            v2 = mine > o2 ? mine : o2;
            v1 = o1;
            j1 = oj;
        } else if (o1 > v2) {
            v2 = o1;
        }
    }
}

// The identities of the probes of group blockIdx.x, rows off[g] .. off[g + 1] of the score matrix.
// ident: the identity or -1; score: the assigned pair's, or of an unknown row its highest over the ok
// identities; second: the row's highest over the ok identities other than the reported one (of an
// unknown row: other than the first that reaches `score`), NaN when there is none.
__global__ __launch_bounds__(CL_TPB) void k_ident_assign(
        const double* __restrict__ score, const int* __restrict__ okp, const int* __restrict__ okg,
        const int* __restrict__ off, int G, double threshold, int exclusive, int* __restrict__ ident,
        double* __restrict__ out_score, double* __restrict__ out_second, const int* err) {
    __shared__ double rb_val[CL_MAX_N];
    __shared__ int rb_j[CL_MAX_N];
    __shared__ unsigned char state[CL_MAX_N];
    __shared__ unsigned closed[ID_MAX_G / 32];
    __shared__ double red_v[CL_TPB / WAVE];
    __shared__ int red_i[CL_TPB / WAVE];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    constexpr int NW = CL_TPB / WAVE;
    const int r0 = off[blockIdx.x];
    int n = off[blockIdx.x + 1] - r0;
    if (n > CL_MAX_N) n = CL_MAX_N;                                     // (the entry point refuses more rows)
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (*err & ERR_NONFINITE) {                                         // (uniform) the matrix is not finite
        for (int i = tid; i < n; i += CL_TPB) {
            ident[r0 + i] = -1;
            out_score[r0 + i] = out_second[r0 + i] = nan;
        }
        return;
    }
    // an identity that is not ok is a closed column from the start
    for (int w = tid; w < (G + 31) / 32; w += CL_TPB) {
        unsigned bits = 0u;
        for (int k = 0; k < 32; ++k) {
            const int j = w * 32 + k;
            if (j >= G || !okg[j]) bits |= 1u << k;
        }
        closed[w] = bits;
    }
    __syncthreads();
    // every row's best column and its two outputs as long as the row stays unknown
    for (int i = wave; i < n; i += NW) {
        double v1 = -INFINITY, v2 = -INFINITY;
        int j1 = -1;
        const int good = okp[r0 + i];                                   // (wave-uniform)
        if (good) ident_row_scan(score + (long long)(r0 + i) * G, closed, G, lane, v1, j1, v2);
        if (lane == 0) {
            rb_val[i] = v1;
            rb_j[i] = j1;
            state[i] = good ? ID_OPEN : 0;
            ident[r0 + i] = -1;
            out_score[r0 + i] = j1 >= 0 ? v1 : nan;
            out_second[r0 + i] = v2 > -INFINITY ? v2 : nan;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (!exclusive) {                                                   // (uniform) every row its own arg-max
        for (int i = tid; i < n; i += CL_TPB)
            if (rb_j[i] >= 0 && rb_val[i] > threshold) ident[r0 + i] = rb_j[i];
        return;
    }
    while (true) {
        // the best pair: the highest value, the first in row-major order on a tie
        double best = -INFINITY;
        int bi = -1;
        for (int i = tid; i < n; i += CL_TPB)
            if (rb_j[i] >= 0 && (bi < 0 || rb_val[i] > best)) { best = rb_val[i]; bi = i; }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(best, m);
            const int oi = __shfl_xor(bi, m);
            if (oi >= 0 && (bi < 0 || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = best; red_i[wave] = bi; }
        __syncthreads();
        best = red_v[0];
        bi = red_i[0];
        for (int w = 1; w < NW; ++w) {
            const double ov = red_v[w];
            const int oi = red_i[w];
            if (oi >= 0 && (bi < 0 || ov > best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if (bi < 0 || !(best > threshold)) break;                       // (uniform) the rows left over are unknown
        const int a = bi, b = rb_j[a];
        __syncthreads();                                                // (red_* and rb_j[a] are read)
        for (int i = tid; i < n; i += CL_TPB)
            if (i != a && rb_j[i] == b) state[i] |= ID_RESCAN;
        if (tid == 0) {
            // the row's highest is v1 = out_score: another column was reported, so v1 is the runner-up
            const double v1 = out_score[r0 + a];
            if (best != v1) { out_second[r0 + a] = v1; out_score[r0 + a] = best; }
            ident[r0 + a] = b;
            state[a] = 0;
            rb_j[a] = -1;
            rb_val[a] = -INFINITY;
            closed[b >> 5] |= 1u << (b & 31);
        }
        __threadfence_block();
        __syncthreads();
        for (int i = wave; i < n; i += NW)
            if (state[i] & ID_RESCAN) {                                 // (wave-uniform)
                double v1, v2;
                int j1;
                ident_row_scan(score + (long long)(r0 + i) * G, closed, G, lane, v1, j1, v2);
                if (lane == 0) {
                    rb_val[i] = v1;
                    rb_j[i] = j1;
                    state[i] &= (unsigned char)~ID_RESCAN;
                }
            }
        __syncthreads();
    }
}

// dst[slot[k]] = (keep[k] ? dst[slot[k]] : 0) + src[member[set_off[k]]] + src[member[set_off[k] + 1]] + ...
__global__ __launch_bounds__(ID_ACC_TPB) void k_bw_accumulate(const double* __restrict__ src,
                                                              const long long* __restrict__ set_off,
                                                              const int* __restrict__ member, const int* __restrict__ slot,
                                                              const int* __restrict__ keep, int E, double* dst) {
    const int k = blockIdx.x, e = threadIdx.x;
    if (e >= E) return;
    double* out = dst + (long long)slot[k] * E + e;
    double acc = keep[k] ? *out : 0.0;
    for (long long m = set_off[k]; m < set_off[k + 1]; ++m) acc = acc + src[(long long)member[m] * E + e];
    *out = acc;
}

}  // namespace spkd
