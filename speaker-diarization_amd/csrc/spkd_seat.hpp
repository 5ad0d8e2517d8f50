// Seats from the delay stream (include/spkd.h (6b4)): the test that two delay records of one file come from two
// places, one best cut per frame range by it (spkd_tdoa_cuts), and one agglomerative chain per group of records
// by it (spkd_tdoa_split).  PARITY: no reference counterpart; tests/seat_numpy.py restates every rule.
//
// A record is spkd_tdoa_stats': int64 [8][3], per channel (n, sum x, sum x^2), in frames.  For a file with
//   w       = (double)(H * rate_out) / (double)(hop * rate_in)      frames per step (the products in int64),
//   floor_f = (floor_s * (double)rate_in)^2                          as k_tdoa_models forms it,
// one channel of a record gives, every operation rounded on its own (no contraction), in this order:
//   dn = (double)n;  mean = (double)sx / dn;  v = (double)sxx / dn - mean * mean;  var = v > floor_f ? v : floor_f;
//   g = dn * log(var).
// For two records A and B, channel c counts iff n_A,c >= min_frames and n_B,c >= min_frames; the reference
// channel and channels >= C never count.  Over the counted channels, ascending, starting from d = 0.0:
//   t = g(A_c + B_c) - g(A_c);  t = t - g(B_c);  t = 0.5 * t;  t = t / w;        (A_c + B_c: the exact integer sums)
//   p = (double)(n_A,c + n_B,c) / w;  p = log(p);  p = lambdac * p;
//   d = d + (t - p).
// Delta(A, B) = d; it is undefined when no channel counts.  Delta > threshold: two seats.  The argument order
// matters to the last bit (t): both kernels hand the earlier record first.
//
//   k_tdoa_cuts  : a workgroup per frame range.  The totals of the range first (a lane per step, as k_tdoa_stats
//                  weighs a step), then tiles of SEAT_TPB steps: the tile's delays staged in LDS, an inclusive scan
//                  of the weighted moments in the waves and across them, the prefix before the tile carried in LDS.
//                  Lane k of a tile evaluates the candidate that opens its step; the best of a lane, of a wave, of
//                  the workgroup by (higher Delta, lower frame).  Integers throughout, no atomics.
//   k_tdoa_split : a workgroup per problem, k_clr_chain's shape with an arg-min: a working copy of the records, the
//                  matrix in device scratch (NaN: undefined), per row the best partner to its right in LDS; a step
//                  merges the lowest pair unless its Delta > threshold, adds record b to record a, and computes row
//                  and column a again.
#pragma once
#include "spkd_tdoa.hpp"

namespace spkd {

constexpr int SEAT_MAX_N = 4096;               // records of one problem (SPKD_SEAT_MAX_N): what the chain's LDS holds
constexpr int SEAT_TPB = 256;                  // k_tdoa_cuts: steps per tile
constexpr int SEAT_CHAIN_TPB = 512;            // k_tdoa_split: 8 waves
constexpr int SEAT_REC = TD_MAX_CH * TD_MOM;   // int64 per record
constexpr unsigned char SEAT_ALIVE = 1, SEAT_OK = 2, SEAT_RESCAN = 4;
static_assert(SEAT_MAX_N <= 65536, "positions are 16-bit");

// what the statistic reads of a file
struct SeatFile { double w, floor_f; int C, ref; };

__host__ __device__ inline SeatFile seat_file(const long long* F, const TdoaClock& K, double floor_s) {
#pragma clang fp contract(off)
    SeatFile f;
    f.w = (double)(F[TDF_H] * K.rate_out) / (double)(K.hop * F[TDF_RATE]);
    const double fr = floor_s * (double)F[TDF_RATE];
    f.floor_f = fr * fr;
    f.C = (int)F[TDF_C], f.ref = (int)F[TDF_REF];
    return f;
}

__device__ __forceinline__ double seat_g(long long n, long long sx, long long sxx, double floor_f) {
#pragma clang fp contract(off)
    const double dn = (double)n;
    const double mean = (double)sx / dn;
    const double v = (double)sxx / dn - mean * mean;
    const double var = v > floor_f ? v : floor_f;
    return dn * log(var);
}

// Delta(A, B) of two records (SEAT_REC int64 each) -> defined; *out is written only then
__device__ __forceinline__ bool seat_delta(const long long* A, const long long* B, const SeatFile& f, int min_frames,
                                           double lambdac, double* out) {
#pragma clang fp contract(off)
    double d = 0.0;
    bool any = false;
#pragma unroll
    for (int c = 0; c < TD_MAX_CH; ++c) {
        if (c < f.C && c != f.ref) {
            const long long na = A[TD_MOM * c], nb = B[TD_MOM * c];
            if (na >= min_frames && nb >= min_frames) {
                const long long xa = A[TD_MOM * c + 1], xb = B[TD_MOM * c + 1], qa = A[TD_MOM * c + 2], qb = B[TD_MOM * c + 2];
                double t = seat_g(na + nb, xa + xb, qa + qb, f.floor_f) - seat_g(na, xa, qa, f.floor_f);
                t = t - seat_g(nb, xb, qb, f.floor_f);
                t = 0.5 * t;
                t = t / f.w;
                double p = (double)(na + nb) / f.w;
                p = log(p);
                p = lambdac * p;
                d = d + (t - p);
                any = true;
            }
        }
    }
    if (any) *out = d;
    return any;
}

// ---- cuts: a workgroup per range
__global__ __launch_bounds__(SEAT_TPB) void k_tdoa_cuts(const int32_t* __restrict__ stream, const long long* __restrict__ files,
                                                        TdoaClock K, const long long* __restrict__ begin,
                                                        const long long* __restrict__ end, const int* __restrict__ file,
                                                        long long min_piece, int min_frames, double floor_s, double lambdac,
                                                        double threshold, long long* __restrict__ out_cut,
                                                        double* __restrict__ out_delta) {
    constexpr int NW = SEAT_TPB / WAVE;
    __shared__ int s_x[SEAT_TPB * TD_MAX_CH];              // the packed delays of the tile's steps, step-major
    __shared__ long long s_part[NW][SEAT_REC];             // per wave: its sum of the moments
    __shared__ long long s_tot[SEAT_REC], s_carry[SEAT_REC];   // of the range; of the steps before the tile
    __shared__ double s_bv[NW];
    __shared__ long long s_bt[NW];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const long long* F = files + (long long)file[r] * TD_FILE;
    const long long T = F[TDF_T], H = F[TDF_H], rate = F[TDF_RATE], frame0 = F[TDF_FRAME0];
    const SeatFile sf = seat_file(F, K, floor_s);
    const int C = sf.C, ref = sf.ref;
    const long long b = begin[r] - frame0, e = end[r] - frame0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    long long s0 = 0, s1 = 0;
    if (C > 1 && T > 0 && e > b) {
        s0 = tdoa_step(b, K, H, rate, T);
        s1 = tdoa_step(e - 1, K, H, rate, T);
    }
    if (s1 == s0) {                                        // (uniform) one channel, no step, inside one step: no candidate
        if (tid == 0) { out_cut[r] = -1; out_delta[r] = nan; }
        return;
    }
    const int32_t* xs = stream + F[TDF_OFF];
    // the weighted moments of step s from its delays x (C of them): what k_tdoa_stats adds for the step
    auto moments = [&](long long s, const int* x, long long* v) {
        const long long first = tdoa_first_frame(s, K, H, rate);
        const long long lo = first > b ? first : b;
        long long hi = e;
        if (s < T - 1) {
            const long long next = tdoa_first_frame(s + 1, K, H, rate);
            hi = next < e ? next : e;
        }
        const long long w = hi > lo ? hi - lo : 0;
#pragma unroll
        for (int c = 0; c < TD_MAX_CH; ++c) {
            v[TD_MOM * c] = v[TD_MOM * c + 1] = v[TD_MOM * c + 2] = 0;
            if (c < C && c != ref) {
                const int xv = x[c];
                if (xv != TD_NONE) {
                    v[TD_MOM * c] = w;
                    v[TD_MOM * c + 1] = w * xv;
                    v[TD_MOM * c + 2] = w * ((long long)xv * xv);
                }
            }
        }
    };
    long long v[SEAT_REC];
    // the totals
    {
        long long acc[SEAT_REC];
#pragma unroll
        for (int k = 0; k < SEAT_REC; ++k) acc[k] = 0;
        for (long long s = s0 + tid; s <= s1; s += SEAT_TPB) {
            moments(s, xs + s * C, v);
#pragma unroll
            for (int k = 0; k < SEAT_REC; ++k) acc[k] += v[k];
        }
#pragma unroll
        for (int k = 0; k < SEAT_REC; ++k) {
            if (k / TD_MOM < C) {                          // (uniform)
                long long a = acc[k];
                for (int m = 1; m < WAVE; m <<= 1) a += __shfl_xor(a, m);
                if (lane == 0) s_part[wave][k] = a;
            }
        }
        __syncthreads();
        if (tid < SEAT_REC) {
            long long a = 0;
            if (tid / TD_MOM < C)
                for (int w = 0; w < NW; ++w) a += s_part[w][tid];
            s_tot[tid] = a;
            s_carry[tid] = 0;
        }
        __syncthreads();
    }
    double best = 0.0;
    long long bt = -1;                                     // (-1: no candidate of this lane has a defined Delta)
    for (long long ts = s0; ts <= s1; ts += SEAT_TPB) {
        const int nt = (int)(s1 - ts + 1 < SEAT_TPB ? s1 - ts + 1 : SEAT_TPB);
        for (int i = tid; i < nt * C; i += SEAT_TPB) s_x[i] = xs[ts * C + i];
        __syncthreads();
        const bool mine = tid < nt;
        if (mine) {
            moments(ts + tid, s_x + tid * C, v);
        } else {
#pragma unroll
            for (int k = 0; k < SEAT_REC; ++k) v[k] = 0;
        }
        long long left[SEAT_REC];                          // the inclusive scan in the wave, then the steps before this one
#pragma unroll
        for (int k = 0; k < SEAT_REC; ++k) {
            left[k] = 0;
            if (k / TD_MOM < C) {
                long long a = v[k];
                for (int m = 1; m < WAVE; m <<= 1) {
                    const long long o = __shfl_up(a, m);
                    if (lane >= m) a += o;
                }
                if (lane == WAVE - 1) s_part[wave][k] = a;
                left[k] = a - v[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SEAT_REC; ++k) {
            if (k / TD_MOM < C) {
                long long a = s_carry[k];
                for (int w = 0; w < wave; ++w) a += s_part[w][k];
                left[k] += a;
            }
        }
        if (mine && ts + tid > s0) {
            const long long t = tdoa_first_frame(ts + tid, K, H, rate);
            if (t - b >= min_piece && e - t >= min_piece) {
                long long right[SEAT_REC];
#pragma unroll
                for (int k = 0; k < SEAT_REC; ++k) right[k] = s_tot[k] - left[k];
                double d;
                if (seat_delta(left, right, sf, min_frames, lambdac, &d) && (bt < 0 || d > best)) {
                    best = d;
                    bt = t;
                }
            }
        }
        __syncthreads();
        if (tid < SEAT_REC && tid / TD_MOM < C) {
            long long a = s_carry[tid];
            for (int w = 0; w < NW; ++w) a += s_part[w][tid];
            s_carry[tid] = a;
        }
        __syncthreads();
    }
    // the highest Delta, the lowest frame among equals
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(best, m);
        const long long ot = __shfl_xor(bt, m);
        if (ot >= 0 && (bt < 0 || ov > best || (ov == best && ot < bt))) { best = ov; bt = ot; }
    }
    if (lane == 0) { s_bv[wave] = best; s_bt[wave] = bt; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < NW; ++w) {
            const double ov = s_bv[w];
            const long long ot = s_bt[w];
            if (ot >= 0 && (bt < 0 || ov > best || (ov == best && ot < bt))) { best = ov; bt = ot; }
        }
        out_delta[r] = bt >= 0 ? best : nan;
        out_cut[r] = (bt >= 0 && best > threshold) ? bt + frame0 : -1;
    }
}

// ---- split: a workgroup per problem
// the best live placed partner to the right of row i, by one wave: the lowest defined value, the lowest column on a tie
__device__ inline void seat_row_scan(const double* mat, const unsigned char* state, int n, int i, int lane, double* rb_val,
                                     int* rb_j) {
    double best = 0.0;
    int bj = -1;
    if ((state[i] & (SEAT_ALIVE | SEAT_OK)) == (SEAT_ALIVE | SEAT_OK)) {      // (wave-uniform)
        for (int j = i + 1 + lane; j < n; j += WAVE)
            if ((state[j] & (SEAT_ALIVE | SEAT_OK)) == (SEAT_ALIVE | SEAT_OK)) {
                const double v = mat[(long long)i * n + j];
                if (v == v && (bj < 0 || v < best)) { best = v; bj = j; }
            }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(best, m);
            const int oj = __shfl_xor(bj, m);
            if (oj >= 0 && (bj < 0 || ov < best || (ov == best && oj < bj))) { best = ov; bj = oj; }
        }
    }
    if (lane == 0) { rb_val[i] = best; rb_j[i] = bj; }
}

__global__ __launch_bounds__(SEAT_CHAIN_TPB) void k_tdoa_split(
        const long long* __restrict__ stats, const long long* __restrict__ files, TdoaClock K,
        const long long* __restrict__ off, const int* __restrict__ prob_file, const long long* __restrict__ mat_off,
        int min_frames, double floor_s, double lambdac, double threshold, long long* W, double* mat_all,
        int* __restrict__ merge_a, int* __restrict__ merge_b, double* __restrict__ merge_d, int* __restrict__ n_merges,
        int* __restrict__ placed) {
    constexpr int NW = SEAT_CHAIN_TPB / WAVE;
    __shared__ double rb_val[SEAT_MAX_N];
    __shared__ int rb_j[SEAT_MAX_N];
    __shared__ unsigned short pos[SEAT_MAX_N];
    __shared__ unsigned char state[SEAT_MAX_N];
    __shared__ double red_v[NW];
    __shared__ int red_i[NW];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    const long long o = off[p];
    const int n = (int)(off[p + 1] - o);
    if (n == 0) {                                                            // (uniform)
        if (tid == 0) n_merges[p] = 0;
        return;
    }
    const SeatFile sf = seat_file(files + (long long)prob_file[p] * TD_FILE, K, floor_s);
    long long* R = W + o * SEAT_REC;                                         // the working copy of the problem's records
    double* mat = mat_all + mat_off[p];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = tid; i < n * SEAT_REC; i += SEAT_CHAIN_TPB) R[i] = stats[o * SEAT_REC + i];
    for (int i = tid; i < n; i += SEAT_CHAIN_TPB) {
        bool ok = false;
        for (int c = 0; c < TD_MAX_CH; ++c)
            if (c < sf.C && c != sf.ref && stats[(o + i) * SEAT_REC + TD_MOM * c] >= min_frames) ok = true;
        if (sf.C < 2) ok = false;
        placed[o + i] = ok ? 1 : 0;
        state[i] = SEAT_ALIVE | (ok ? SEAT_OK : 0);
        pos[i] = (unsigned short)i;
    }
    __threadfence_block();
    __syncthreads();
    if (n == 1) {
        if (tid == 0) n_merges[p] = 0;
        return;
    }
    for (long long e = tid; e < (long long)n * n; e += SEAT_CHAIN_TPB) {
        const int i = (int)(e / n), j = (int)(e - (long long)i * n);
        if (j > i && (state[i] & SEAT_OK) && (state[j] & SEAT_OK)) {
            double d;
            mat[e] = seat_delta(R + (long long)i * SEAT_REC, R + (long long)j * SEAT_REC, sf, min_frames, lambdac, &d) ? d : nan;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int i = wave; i < n; i += NW) seat_row_scan(mat, state, n, i, lane, rb_val, rb_j);
    int nm = 0;
    while (true) {
        __syncthreads();
        // the best pair: the lowest value, the first in row-major order on a tie
        double best = 0.0;
        int bi = -1;
        for (int i = tid; i < n; i += SEAT_CHAIN_TPB)
            if (rb_j[i] >= 0 && (bi < 0 || rb_val[i] < best)) { best = rb_val[i]; bi = i; }
#pragma unroll
        for (int m = WAVE / 2; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(best, m);
            const int oi = __shfl_xor(bi, m);
            if (oi >= 0 && (bi < 0 || ov < best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = best; red_i[wave] = bi; }
        __syncthreads();
        best = red_v[0];
        bi = red_i[0];
        for (int w = 1; w < NW; ++w) {
            const double ov = red_v[w];
            const int oi = red_i[w];
            if (oi >= 0 && (bi < 0 || ov < best || (ov == best && oi < bi))) { best = ov; bi = oi; }
        }
        if (bi < 0) break;                                                   // (uniform) no pair has a defined Delta
        if (best > threshold) break;                                         // two seats: the chain stops
        const int a = bi, b = rb_j[a];
        __syncthreads();                                                     // (red_* and rb_j[a] are read)
        if (tid == 0) {
            merge_a[o + nm] = pos[a];
            merge_b[o + nm] = pos[b];
            merge_d[o + nm] = best;
        }
        ++nm;
        if (tid < SEAT_REC) R[(long long)a * SEAT_REC + tid] += R[(long long)b * SEAT_REC + tid];
        for (int s = b + 1 + tid; s < n; s += SEAT_CHAIN_TPB) pos[s] -= 1;
        if (tid == 0) {
            state[b] = 0;
            state[a] |= SEAT_RESCAN;
            rb_j[b] = -1;
        }
        __threadfence_block();
        __syncthreads();
        // row and column a; what that means for the best partner of the other rows
        for (int x = tid; x < n; x += SEAT_CHAIN_TPB) {
            if (x == a || (state[x] & (SEAT_ALIVE | SEAT_OK)) != (SEAT_ALIVE | SEAT_OK)) continue;
            const int lo = x < a ? x : a, hi = x < a ? a : x;
            double d;
            const bool def = seat_delta(R + (long long)lo * SEAT_REC, R + (long long)hi * SEAT_REC, sf, min_frames, lambdac, &d);
            mat[(long long)lo * n + hi] = def ? d : nan;
            const int j = rb_j[x];
            if (j == b || (x < a && j == a)) state[x] |= SEAT_RESCAN;
            else if (x < a && def && (j < 0 || d < rb_val[x] || (d == rb_val[x] && a < j))) { rb_val[x] = d; rb_j[x] = a; }
        }
        __threadfence_block();
        __syncthreads();
        for (int x = wave; x < n; x += NW)
            if (state[x] & SEAT_RESCAN) {                                    // (wave-uniform)
                seat_row_scan(mat, state, n, x, lane, rb_val, rb_j);
                if (lane == 0) state[x] &= (unsigned char)~SEAT_RESCAN;
            }
    }
    if (tid == 0) n_merges[p] = nm;
}

}  // namespace spkd
