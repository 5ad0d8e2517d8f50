// Agglomerative linking of speaker records (spkd_ubm_stats.hpp) by cross-likelihood ratio under
// MAP-adapted means, the whole chain on the device in one call (spkd_clr_link).
// PARITY: no reference counterpart -- the reference links nothing across files; tests/link_clr_numpy.py
// restates the scores and the chain in numpy.
//
// With the UBM's means mu and inverse variances, the relevance r and a record R = (n_c, f_c):
//   m_c = (f_c + r mu_c) / (n_c + r),  N = sum_c n_c (component order),
//   H(a|b) = (1 / N_a) sum_c sum_d [(m^b_cd - mu_cd) f^a_cd - 1/2 n^a_c ((m^b_cd)^2 - mu_cd^2)] / var_cd.
// Per cluster b the factors of a's record are kept as a derived record T_b of the same shape,
//   T_b[c][0] = -sum_d 1/2 ((m^b_cd)^2 - mu_cd^2) / var_cd,  T_b[c][1 + d] = (m^b_cd - mu_cd) / var_cd,
// so that H(a|b) = (R_a . T_b) / N_a, one dot product of C * 40 terms, and
// CLR(a, b) = H(a|b) + H(b|a) for a < b.
//
//   k_clr_prep   : a wave per speaker: the working copy of its record, N and T.
//   k_clr_matrix : a workgroup per row a of the initial matrix, 16 lanes per pair (a, b > a): coalesced
//                  reads of both records, a butterfly over the 16 partial sums.
//   k_clr_chain  : ONE workgroup walks the chain.  Per row the best partner to its right waits in LDS;
//                  a step is an arg-max over those, the merge (record a += record b, T_a, N_a), row and
//                  column a recomputed (16 lanes per partner), and a new scan of the rows whose best
//                  partner was a or b.  Clusters keep their slot; a slot's position in the shrinking
//                  list (what the log states: speakers.pop(b)) is counted down in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"
#include "spkd_gmm_train.hpp"
#include "spkd_ubm_stats.hpp"

namespace spkd {

constexpr int CL_MAX_N = 4096;        // speakers of one call (SPKD_CLR_MAX_N): what the chain's LDS holds
constexpr int CL_TPB = 1024;          // k_clr_chain: 16 waves
constexpr int CL_GROUP = 16;          // lanes per pair
constexpr int CL_MAT_TPB = 256;       // k_clr_matrix
constexpr unsigned char CL_ALIVE = 1, CL_OK = 2, CL_RESCAN = 4;
static_assert(CL_MAX_N <= 65536, "positions are 16-bit");

// T and N of the record R (K components of BW_COMP doubles), by the nt threads of a workgroup; R is
// complete and visible before the call, T and N are after the caller's next barrier
__device__ inline void clr_derive(const double* R, const double* __restrict__ ubm, int K, double r, double* T,
                                  double* N, int tid, int nt) {
    for (int e = tid; e < K * BW_COMP; e += nt) {
        const int c = e / BW_COMP, d = e - c * BW_COMP - 1;
        const double* __restrict__ U = ubm + c * GT_COMP;
        const double den = R[c * BW_COMP] + r;
        if (d >= 0) {
            const double m = (R[e] + r * U[GT_MEAN + d]) / den;
            T[e] = (m - U[GT_MEAN + d]) * U[GT_IVAR + d];
        } else {
            double q = 0.0;
            for (int j = 0; j < D; ++j) {
                const double mu = U[GT_MEAN + j];
                const double m = (R[c * BW_COMP + 1 + j] + r * mu) / den;
                q += 0.5 * (m * m - mu * mu) * U[GT_IVAR + j];
            }
            T[e] = -q;
        }
    }
    if (tid == 0) {
        double n = 0.0;
        for (int c = 0; c < K; ++c) n += R[c * BW_COMP];
        *N = n;
    }
}

// CLR(lo, hi) by the 16 lanes of a group (sub: the lane's place in it); the same value in each
__device__ inline double clr_pair(const double* Rl, const double* Tl, double Nl, const double* Rh, const double* Th,
                                  double Nh, int E, int sub) {
    double hl = 0.0, hh = 0.0;
    for (int e = sub; e < E; e += CL_GROUP) {
        hl = fma(Rl[e], Th[e], hl);
        hh = fma(Rh[e], Tl[e], hh);
    }
#pragma unroll
    for (int m = CL_GROUP / 2; m >= 1; m >>= 1) {
        hl += __shfl_xor(hl, m, CL_GROUP);
        hh += __shfl_xor(hh, m, CL_GROUP);
    }
    return hl / Nl + hh / Nh;
}

__global__ __launch_bounds__(WAVE) void k_clr_prep(const double* __restrict__ bw, const double* __restrict__ ubm, int K,
                                                   double r, double* W, double* T, double* Nn) {
    const long long s = blockIdx.x;
    const int E = K * BW_COMP;
    for (int e = threadIdx.x; e < E; e += WAVE) W[s * E + e] = bw[s * E + e];
    __syncthreads();
    clr_derive(W + s * E, ubm, K, r, T + s * E, Nn + s, threadIdx.x, WAVE);
}

__global__ __launch_bounds__(CL_MAT_TPB) void k_clr_matrix(const double* __restrict__ W, const double* __restrict__ T,
                                                           const double* __restrict__ Nn, const int* __restrict__ ok,
                                                           int n, int K, double* __restrict__ mat, int* err) {
    const int a = blockIdx.x;
    if (!ok[a]) return;                                                 // (uniform)
    const int E = K * BW_COMP;
    const int sub = threadIdx.x % CL_GROUP, g = threadIdx.x / CL_GROUP;
    for (int b = a + 1 + g; b < n; b += CL_MAT_TPB / CL_GROUP) {
        if (!ok[b]) continue;                                           // (uniform in the group)
        const double v = clr_pair(W + (long long)a * E, T + (long long)a * E, Nn[a], W + (long long)b * E,
                                  T + (long long)b * E, Nn[b], E, sub);
        if (sub == 0) {
            mat[(long long)a * n + b] = v;
            if (!gt_finite(v)) atomicOr(err, ERR_NONFINITE);
        }
    }
}

// the best live ok partner to the right of row i, by one wave: the highest value, the lowest column on
// a tie; vmax / vmin take in the values seen (the statistics of the initial matrix)
__device__ inline void clr_row_scan(const double* mat, const unsigned char* state, int n, int i, int lane,
                                    double* rb_val, int* rb_j, double& vmax, double& vmin) {
    double best = -INFINITY;
    int bj = -1;
    if ((state[i] & (CL_ALIVE | CL_OK)) == (CL_ALIVE | CL_OK)) {        // (wave-uniform)
        for (int j = i + 1 + lane; j < n; j += WAVE)
            if ((state[j] & (CL_ALIVE | CL_OK)) == (CL_ALIVE | CL_OK)) {
                const double v = mat[(long long)i * n + j];
                if (v > best) { best = v; bj = j; }
                if (v > vmax || vmax != vmax) vmax = v;                 // (NaN: nothing seen yet)
                if (v < vmin || vmin != vmin) vmin = v;
            }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(best, m);
            const int oj = __shfl_xor(bj, m);
            if (oj >= 0 && (bj < 0 || ov > best || (ov == best && oj < bj))) { best = ov; bj = oj; }
        }
    }
    if (lane == 0) { rb_val[i] = best; rb_j[i] = bj; }
}

__global__ __launch_bounds__(CL_TPB) void k_clr_chain(
        double* W, double* T, double* Nn, double* mat, const int* __restrict__ ok, int n, int K,
        const double* __restrict__ ubm, double r, double threshold, int max_spk, int* __restrict__ merge_a,
        int* __restrict__ merge_b, double* __restrict__ merge_d, int* __restrict__ n_merges, double* __restrict__ stat,
        int* err) {
    __shared__ double rb_val[CL_MAX_N];
    __shared__ int rb_j[CL_MAX_N];
    __shared__ unsigned short pos[CL_MAX_N];
    __shared__ unsigned char state[CL_MAX_N];
    __shared__ double red_v[CL_TPB / WAVE], red_w[CL_TPB / WAVE];
    __shared__ int red_i[CL_TPB / WAVE];
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    constexpr int NW = CL_TPB / WAVE;
    const int E = K * BW_COMP;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (*err & ERR_NONFINITE) {                                         // (uniform) the initial matrix is not finite
        if (tid == 0) { *n_merges = 0; stat[0] = stat[1] = nan; }
        return;
    }
    for (int i = tid; i < n; i += CL_TPB) {
        state[i] = CL_ALIVE | (ok[i] ? CL_OK : 0);
        pos[i] = (unsigned short)i;
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    double vmax = nan, vmin = nan;
    for (int i = wave; i < n; i += NW) clr_row_scan(mat, state, n, i, lane, rb_val, rb_j, vmax, vmin);
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const double a = __shfl_xor(vmax, m), b = __shfl_xor(vmin, m);
        if (a > vmax || vmax != vmax) vmax = a;
        if (b < vmin || vmin != vmin) vmin = b;
    }
    if (lane == 0) { red_v[wave] = vmax; red_w[wave] = vmin; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) {
            if (red_v[w] > vmax || vmax != vmax) vmax = red_v[w];
            if (red_w[w] < vmin || vmin != vmin) vmin = red_w[w];
        }
        stat[0] = vmax;
        stat[1] = vmin;
    }
    int live = n, nm = 0;
    double dummy_max = nan, dummy_min = nan;
    while (true) {
        __syncthreads();
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
        if (bi < 0) break;                                              // (uniform) fewer than two ok clusters
        if (!(best > threshold || (max_spk > 0 && live > max_spk))) break;
        const int a = bi, b = rb_j[a];
        __syncthreads();                                                // (red_* and rb_j[a] are read)
        if (tid == 0) {
            merge_a[nm] = pos[a];
            merge_b[nm] = pos[b];
            merge_d[nm] = best;
        }
        ++nm;
        --live;
        for (int e = tid; e < E; e += CL_TPB) W[(long long)a * E + e] += W[(long long)b * E + e];
        __threadfence_block();
        __syncthreads();
        clr_derive(W + (long long)a * E, ubm, K, r, T + (long long)a * E, Nn + a, tid, CL_TPB);
        for (int s = b + 1 + tid; s < n; s += CL_TPB) pos[s] -= 1;
        if (tid == 0) {
            state[b] = 0;
            state[a] |= CL_RESCAN;
            rb_j[b] = -1;
            rb_val[b] = -INFINITY;
        }
        __threadfence_block();
        __syncthreads();
        // row and column a; what that means for the best partner of the other rows
        const int sub = tid % CL_GROUP;
        for (int x = tid / CL_GROUP; x < n; x += CL_TPB / CL_GROUP) {
            if (x == a || (state[x] & (CL_ALIVE | CL_OK)) != (CL_ALIVE | CL_OK)) continue;   // (uniform in the group)
            const int lo = x < a ? x : a, hi = x < a ? a : x;
            const double v = clr_pair(W + (long long)lo * E, T + (long long)lo * E, Nn[lo], W + (long long)hi * E,
                                      T + (long long)hi * E, Nn[hi], E, sub);
            if (sub == 0) {
                mat[(long long)lo * n + hi] = v;
                if (!gt_finite(v)) bad = 1;
                const int j = rb_j[x];
                if (j == b || (x < a && j == a)) state[x] |= CL_RESCAN;
                else if (x < a && (j < 0 || v > rb_val[x] || (v == rb_val[x] && a < j))) { rb_val[x] = v; rb_j[x] = a; }
            }
        }
        __threadfence_block();
        __syncthreads();
        if (bad) {                                                      // (uniform)
            if (tid == 0) atomicOr(err, ERR_NONFINITE);
            break;
        }
        for (int x = wave; x < n; x += NW)
            if (state[x] & CL_RESCAN) {                                 // (wave-uniform)
                clr_row_scan(mat, state, n, x, lane, rb_val, rb_j, dummy_max, dummy_min);
                if (lane == 0) state[x] &= (unsigned char)~CL_RESCAN;
            }
    }
    if (tid == 0) *n_merges = nm;
}

}  // namespace spkd
