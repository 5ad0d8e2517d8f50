// The delay stream (include/spkd.h (6b3)): the per-step delays of spkd_bf_track kept for a whole batch as
// packed int32, the exact delay statistics of frame sets, one diagonal Gaussian per (speaker, channel)
// from them, and their weighted log-likelihood added to the score matrix of the resegmentation stage.
// The rule that takes a feature frame to its step (tdoa_step) and its inverse (tdoa_first_frame) are
// stated once here, for the host tables and the kernels alike; frontend.DelayStream mirrors them.
#pragma once
#include "spkd_device.hpp"
#include "spkd_gauss.hpp"

namespace spkd {

constexpr int32_t TD_NONE = INT32_MIN;   // a step that is not reliable on a channel (SPKD_TDOA_NONE)
constexpr int TD_MAX_CH = 8;             // channels of a file (SPKD_TDOA_MAX_CH, the beamformer's limit)
constexpr int TD_MAX_DELAY = 4096;       // |delay| of a reliable entry (SPKD_TDOA_MAX_DELAY, the beamformer's largest lag)
constexpr int TD_FILE = 8;               // int64 per file of the host table (SPKD_TDOA_FILE)
constexpr int TD_MOM = 3;                // (n, sum x, sum x^2) per (set, channel)
constexpr int TD_MODEL = 4;              // doubles per (speaker, channel): mean, var, 1 / (2 var), -1/2 log(2 pi var)
constexpr int ERR_TDOA_STEPS = 32;       // internal: a tile of k_tdoa_score spans more steps than its LDS holds
constexpr int TD_TPB = 256;              // lanes of a workgroup: steps of k_tdoa_stats, frames of k_tdoa_score
enum { TDF_OFF = 0, TDF_T, TDF_C, TDF_REF, TDF_H, TDF_RATE, TDF_FRAME0, TDF_RESERVED };

// the frame clock of the features the steps are matched to: hop and window in samples at rate_out
struct TdoaClock { long long hop, window, rate_out; };

// Feature frame t of a file (file-local) belongs to the step
//   min(T - 1, ((t * hop + window / 2) * rate_in) / (rate_out * H)):
// the step whose first input sample, s H, is the last one at or before the centre of the frame's window, the
// last step taking every later frame.  64-bit integers; the caller keeps (t * hop + window / 2) * rate_in
// below 2^63 (tdoa_frame_limit).  T >= 1.
__host__ __device__ inline long long tdoa_step(long long t, const TdoaClock& K, long long H, long long rate_in, long long T) {
    const long long s = ((t * K.hop + K.window / 2) * rate_in) / (K.rate_out * H);
    return s < T - 1 ? s : T - 1;
}

// The first frame of step s under the rule above without its clamp: the smallest t >= 0 with
// (t * hop + window / 2) * rate_in >= s * rate_out * H.  The frames of step s < T - 1 are
// [tdoa_first_frame(s), tdoa_first_frame(s + 1)), those of step T - 1 everything from its first on.  The
// caller keeps s * rate_out * H below 2^63 (tdoa_step_limit).
__host__ __device__ inline long long tdoa_first_frame(long long s, const TdoaClock& K, long long H, long long rate_in) {
    if (s <= 0) return 0;
    const long long a = s * K.rate_out * H;
    const long long q = a / rate_in + (a % rate_in != 0) - K.window / 2;     // the centre sample at rate_out, at the least
    return q <= 0 ? 0 : q / K.hop + (q % K.hop != 0);
}

// the largest file-local frame the rule takes at rate_in, and the largest step count the inverse takes
inline long long tdoa_frame_limit(const TdoaClock& K, long long rate_in) {
    return (INT64_MAX / rate_in - K.window / 2) / K.hop;
}
inline long long tdoa_step_limit(const TdoaClock& K, long long H) { return INT64_MAX / (K.rate_out * H) - 1; }

// ---- pack: one lane per entry
__global__ __launch_bounds__(TD_TPB) void k_tdoa_pack(const int32_t* __restrict__ delay, const float* __restrict__ val,
                                                      float min_peak, long long n, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * TD_TPB + threadIdx.x;
    if (i >= n) return;
    out[i] = val[4 * i] >= min_peak ? delay[i] : TD_NONE;                    // (the first candidate's value: _beamform_group's test)
}

// ---- statistics: a workgroup per (range, run of TD_TPB steps), a lane per step
struct TdoaItem {
    long long b, e;              // the range, in frames of its file
    int file, set, step0, n_steps;
};

__global__ __launch_bounds__(TD_TPB) void k_tdoa_stats(const int32_t* __restrict__ stream, const long long* __restrict__ files,
                                                       TdoaClock K, const TdoaItem* __restrict__ items,
                                                       unsigned long long* __restrict__ out) {
    __shared__ long long part[TD_TPB / WAVE][TD_MAX_CH * TD_MOM];
    const TdoaItem it = items[blockIdx.x];
    const long long* F = files + (long long)it.file * TD_FILE;
    const long long T = F[TDF_T], H = F[TDF_H], rate = F[TDF_RATE];
    const int C = (int)F[TDF_C], ref = (int)F[TDF_REF];
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE;
    long long acc[TD_MAX_CH * TD_MOM];
#pragma unroll
    for (int k = 0; k < TD_MAX_CH * TD_MOM; ++k) acc[k] = 0;
    if (tid < it.n_steps) {
        const long long s = it.step0 + tid;
        const long long first = tdoa_first_frame(s, K, H, rate);
        const long long lo = first > it.b ? first : it.b;
        long long hi = it.e;
        if (s < T - 1) {
            const long long next = tdoa_first_frame(s + 1, K, H, rate);
            hi = next < it.e ? next : it.e;
        }
        const long long w = hi > lo ? hi - lo : 0;       // the frames of the range in this step
        const int32_t* x = stream + F[TDF_OFF] + s * C;
#pragma unroll
        for (int c = 0; c < TD_MAX_CH; ++c) {
            if (c < C && c != ref) {
                const int32_t v = x[c];
                if (v != TD_NONE) {
                    acc[TD_MOM * c] += w;
                    acc[TD_MOM * c + 1] += w * v;
                    acc[TD_MOM * c + 2] += w * ((long long)v * v);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < TD_MAX_CH * TD_MOM; ++k) {
        if (k / TD_MOM < C) {                            // (uniform: the file's channels)
            long long v = acc[k];
            for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m);
            if (lane == 0) part[wave][k] = v;
        }
    }
    __syncthreads();
    if (tid < TD_MAX_CH * TD_MOM && tid / TD_MOM < C) {
        long long v = 0;
        for (int w = 0; w < TD_TPB / WAVE; ++w) v += part[w][tid];
        if (v != 0) atomicAdd(out + (long long)it.set * (TD_MAX_CH * TD_MOM) + tid, (unsigned long long)v);
    }
}

// ---- models: a wave per file, a lane per (speaker of the file, channel)
__global__ __launch_bounds__(WAVE) void k_tdoa_models(const long long* __restrict__ stats, const long long* __restrict__ files,
                                                      const long long* __restrict__ spk_off, const int* __restrict__ ok,
                                                      int min_frames, double floor_s, double* __restrict__ models,
                                                      int* __restrict__ live) {
#pragma clang fp contract(off)
    __shared__ int dead;
    const int f = blockIdx.x, lane = threadIdx.x;
    const long long* F = files + (long long)f * TD_FILE;
    const int C = (int)F[TDF_C], ref = (int)F[TDF_REF];
    const double fr = floor_s * (double)F[TDF_RATE], floor_f = fr * fr;
    if (lane == 0) dead = 0;
    __syncthreads();
    const long long s0 = spk_off[f], n = (spk_off[f + 1] - s0) * TD_MAX_CH;
    for (long long i = lane; i < n; i += WAVE) {
        const long long s = s0 + i / TD_MAX_CH;
        const int c = (int)(i % TD_MAX_CH);
        double mean = 0.0, var = floor_f, inv = 0.0, ln = 0.0;       // the neutral model: it adds 0 to every score
        if (C > 1 && c < C && c != ref) {
            const long long* st = stats + (s * TD_MAX_CH + c) * TD_MOM;
            const long long cnt = st[0];
            if (cnt >= min_frames) {
                const double dn = (double)cnt;
                mean = (double)st[1] / dn;
                const double v = (double)st[2] / dn - mean * mean;
                var = v > floor_f ? v : floor_f;
                inv = 1.0 / (2.0 * var);
                ln = -0.5 * log(6.283185307179586 * var);
            } else if (ok[s]) {
                atomicOr(&dead, 1 << c);
            }
        }
        double* m = models + (s * TD_MAX_CH + c) * TD_MODEL;
        m[0] = mean, m[1] = var, m[2] = inv, m[3] = ln;
    }
    __syncthreads();
    if (lane == 0) live[f] = C > 1 ? (((1 << C) - 1) & ~(1 << ref) & ~dead) : 0;
}

// ---- scores: a workgroup per tile of TD_TPB frames of one sequence
struct TdoaSeqs {
    const long long *begin, *end, *row, *tile;   // per sequence: frames [begin, end) of the batch, first row of the scores, first tile
    const int *file, *model, *n_models;          // its file, its first model and its model count
    const int *tile_seq, *live;                  // per tile its sequence; per file its live channels
};

// one entry: val + weight * ll in fp64, rounded once; a value that is not finite and a column past the
// sequence's models stay what they are
__device__ __forceinline__ float tdoa_fuse(float val, int e, int n_cols, int nm, int C, int mask, double weight,
                                           const int* s_x, const unsigned short* s_step, const double* s_m) {
#pragma clang fp contract(off)
    const int fr = e / n_cols, col = e - fr * n_cols;
    if (col >= nm || !(fabsf(val) < INFINITY)) return val;
    const int* x = s_x + (int)s_step[fr] * C;
    const double* m = s_m + col * (TD_MAX_CH * 3);
    double ll = 0.0;
    for (int c = 0; c < C; ++c) {
        const int xv = x[c];
        if (((mask >> c) & 1) && xv != TD_NONE) {
            const double d = (double)xv - m[3 * c];
            double t = d * d;
            t = t * m[3 * c + 1];
            ll = ll + (m[3 * c + 2] - t);
        }
    }
    const double add = weight * ll;
    return (float)((double)val + add);
}

__global__ __launch_bounds__(TD_TPB) void k_tdoa_score(const int32_t* __restrict__ stream, const long long* __restrict__ files,
                                                       TdoaClock K, const double* __restrict__ models, TdoaSeqs S, int n_cols,
                                                       double weight, float* __restrict__ scores, int* __restrict__ err) {
    __shared__ int s_x[TD_TPB * TD_MAX_CH];                  // the packed delays of the tile's steps, step-major
    __shared__ double s_m[GS_MAX_COLS * TD_MAX_CH * 3];      // mean, 1 / (2 var), log term per (column, channel)
    __shared__ unsigned short s_step[TD_TPB];                // per frame of the tile its step, from the tile's first
    __shared__ long long s_first;
    const int tid = threadIdx.x;
    const int q = S.tile_seq[blockIdx.x];
    const long long k = (long long)blockIdx.x - S.tile[q];
    const long long f0 = S.begin[q] + k * TD_TPB;
    const int nf = (int)(S.end[q] - f0 < TD_TPB ? S.end[q] - f0 : TD_TPB);
    const int file = S.file[q], nm = S.n_models[q], mask = S.live[file];
    const long long* F = files + (long long)file * TD_FILE;
    const long long T = F[TDF_T], H = F[TDF_H], rate = F[TDF_RATE];
    const int C = (int)F[TDF_C];
    long long st = 0;
    if (tid < nf) st = tdoa_step(f0 - F[TDF_FRAME0] + tid, K, H, rate, T);
    if (tid == 0) s_first = st;
    __syncthreads();
    const long long first = s_first;
    const long long rel = st - first;
    if (tid < nf) s_step[tid] = (unsigned short)(rel < TD_TPB ? rel : TD_TPB);
    __syncthreads();
    const int n_steps = (int)s_step[nf - 1] + 1;
    if (n_steps > TD_TPB) {                                  // (a step shorter than a frame: the host refuses it)
        if (tid == 0) atomicOr(err, ERR_TDOA_STEPS);
        return;
    }
    const int32_t* x = stream + F[TDF_OFF] + first * C;
    for (int i = tid; i < n_steps * C; i += TD_TPB) s_x[i] = x[i];
    for (int i = tid; i < nm * TD_MAX_CH * 3; i += TD_TPB) {
        const int col = i / (TD_MAX_CH * 3), r = i % (TD_MAX_CH * 3), c = r / 3, m = r % 3;
        s_m[i] = models[(((long long)S.model[q] + col) * TD_MAX_CH + c) * TD_MODEL + (m == 0 ? 0 : m + 1)];
    }
    __syncthreads();
    // the tile's entries are contiguous: single floats up to a 16-byte border, float4 pieces, single floats
    float* p = scores + (S.row[q] + k * TD_TPB) * n_cols;
    const int count = nf * n_cols;
    int head = (int)((16 - ((uintptr_t)p & 15)) & 15) / 4;
    if (head > count) head = count;
    const int n_vec = (count - head) / 4, tail = head + 4 * n_vec;
    if (tid < head) p[tid] = tdoa_fuse(p[tid], tid, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
    float4* pv = reinterpret_cast<float4*>(p + head);
    for (int v = tid; v < n_vec; v += TD_TPB) {
        float4 r = pv[v];
        const int e = head + 4 * v;
        r.x = tdoa_fuse(r.x, e, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
        r.y = tdoa_fuse(r.y, e + 1, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
        r.z = tdoa_fuse(r.z, e + 2, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
        r.w = tdoa_fuse(r.w, e + 3, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
        pv[v] = r;
    }
    if (tid < count - tail) p[tail + tid] = tdoa_fuse(p[tail + tid], tail + tid, n_cols, nm, C, mask, weight, s_x, s_step, s_m);
}

}  // namespace spkd
