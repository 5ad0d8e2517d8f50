// Overlapped speech from the delay stream (include/spkd.h (6b5)): the runner-up lag of every step and channel kept
// as a second stream (spkd_tdoa_second), and per step the pair of speakers whose seats the tracked delay and the
// runner-up name on enough channels (spkd_tdoa_overlap).  PARITY: no reference counterpart; tests/overlap_numpy.py
// restates every rule.
//
// The near rule, stated once (ovl_near): a lag x is near speaker j on channel c iff, with (mean, ., inv2var, .) the
// model of (j, c) as k_tdoa_models left it and every operation rounded on its own (no contraction),
//   d = (double)x - mean;  t = d * d;  t = t * inv2var;  t <= gate.
//
//   k_tdoa_second : a lane per entry.  The first slot k < n_best with a finite value and |lag - delay| > guard is the
//                   runner-up; its lag is written iff its value >= min_second, TD_NONE otherwise and when the step is
//                   not reliable (val[4 i] < min_peak).  The reference channel's entry has one finite slot, its own
//                   delay, so it is TD_NONE by the same walk.
//   k_ovl_match   : a workgroup per tile of OVL_TPB steps of one file, a lane per step.  The file's models (mean,
//                   inv2var per speaker and channel) go into LDS once.  Per live channel two 16-bit masks: the speakers
//                   the tracked delay is near, the speakers the runner-up is near; channel c agrees with (j, k) iff
//                   (P_c[j] and Q_c[k]) or (Q_c[j] and P_c[k]).  The pairs j < k are walked in lexicographic order, the
//                   first with the largest count wins.  The raw pair is one int32: j | k << 8, or -1.
//   k_ovl_runs    : the same grid.  A step keeps its raw pair iff the run of equal raw pairs around it inside its
//                   file is at least min_steps long; a lane reads at most min_steps - 1 neighbours on each side.
// No atomics; what a step gets depends on its file alone.
#pragma once
#include "spkd_tdoa.hpp"

namespace spkd {

constexpr int OVL_TPB = 256;                   // steps per workgroup of both kernels
constexpr int OVL_MAX_SPK = 16;                // speakers of a file (SPKD_OVERLAP_MAX_SPK): a mask is 16 bits
constexpr int OVL_MAX_RUN = 64;                // the largest min_steps (SPKD_OVERLAP_MAX_RUN)

__host__ __device__ inline bool ovl_near(int x, double mean, double inv2var, double gate) {
#pragma clang fp contract(off)
    const double d = (double)x - mean;
    double t = d * d;
    t = t * inv2var;
    return t <= gate;
}

// ---- the runner-up stream: one lane per entry
__global__ __launch_bounds__(TD_TPB) void k_tdoa_second(const int32_t* __restrict__ delay, const int32_t* __restrict__ lag,
                                                        const float* __restrict__ val, int n_best, float min_peak,
                                                        float min_second, int guard, long long n, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * TD_TPB + threadIdx.x;
    if (i >= n) return;
    int32_t r = TD_NONE;
    if (val[4 * i] >= min_peak) {
        const long long d = delay[i];
        for (int k = 0; k < n_best; ++k) {
            const float v = val[4 * i + k];
            const long long off = (long long)lag[4 * i + k] - d;
            if (fabsf(v) < INFINITY && (off > guard || -off > guard)) {
                if (v >= min_second) r = lag[4 * i + k];
                break;
            }
        }
    }
    out[i] = r;
}

// ---- the pair of every step
struct OvlTile { int file, step0; };

struct OvlFiles {
    const long long *files, *spk_off, *step_off;   // the stream's table; per file its first model; its first step of d_pair
    const int* live;                               // per file the live channels, as k_tdoa_models left them
};

__global__ __launch_bounds__(OVL_TPB) void k_ovl_match(const int32_t* __restrict__ stream, const int32_t* __restrict__ second,
                                                       OvlFiles S, const OvlTile* __restrict__ tiles,
                                                       const double* __restrict__ models, double gate, int min_channels,
                                                       int32_t* __restrict__ raw) {
    __shared__ double s_m[OVL_MAX_SPK * TD_MAX_CH * 2];            // mean, inv2var per (speaker, channel)
    const OvlTile tl = tiles[blockIdx.x];
    const long long* F = S.files + (long long)tl.file * TD_FILE;
    const long long T = F[TDF_T];
    const int C = (int)F[TDF_C], ref = (int)F[TDF_REF], tid = threadIdx.x;
    const long long m0 = S.spk_off[tl.file];
    const int n_spk = (int)(S.spk_off[tl.file + 1] - m0);
    const int live = C > 1 ? (S.live[tl.file] & ((1 << C) - 1) & ~(1 << ref)) : 0;
    const int need = min(min_channels, __popc(live));
    const long long t = (long long)tl.step0 + tid;
    if (n_spk < 2 || need < 1) {                                   // (uniform) one speaker, one channel, no live channel
        if (t < T) raw[S.step_off[tl.file] + t] = -1;
        return;
    }
    for (int i = tid; i < n_spk * TD_MAX_CH * 2; i += OVL_TPB) {
        const int sc = i / 2;
        s_m[i] = models[(m0 * TD_MAX_CH + sc) * TD_MODEL + (i % 2 ? 2 : 0)];
    }
    __syncthreads();
    if (t >= T) return;
    const int32_t* x = stream + F[TDF_OFF] + t * C;
    const int32_t* y = second + F[TDF_OFF] + t * C;
    unsigned P[TD_MAX_CH], Q[TD_MAX_CH];
    int any = 0;
#pragma unroll
    for (int c = 0; c < TD_MAX_CH; ++c) {
        P[c] = Q[c] = 0;
        if (c < C && ((live >> c) & 1)) {
            const int32_t p = x[c], q = y[c];
            if (p != TD_NONE && q != TD_NONE) {
                for (int j = 0; j < n_spk; ++j) {
                    const double mean = s_m[(j * TD_MAX_CH + c) * 2], inv = s_m[(j * TD_MAX_CH + c) * 2 + 1];
                    P[c] |= (unsigned)ovl_near(p, mean, inv, gate) << j;
                    Q[c] |= (unsigned)ovl_near(q, mean, inv, gate) << j;
                }
                any |= (P[c] != 0) & (Q[c] != 0);
            }
        }
    }
    int best = 0, pair = -1;
    if (any) {
        for (int j = 0; j + 1 < n_spk; ++j) {
            for (int k = j + 1; k < n_spk; ++k) {
                int n = 0;
#pragma unroll
                for (int c = 0; c < TD_MAX_CH; ++c)
                    n += (int)((((P[c] >> j) & (Q[c] >> k)) | ((Q[c] >> j) & (P[c] >> k))) & 1u);
                if (n > best) { best = n; pair = j | (k << 8); }
            }
        }
    }
    raw[S.step_off[tl.file] + t] = best >= need ? pair : -1;
}

// ---- the run filter
__global__ __launch_bounds__(OVL_TPB) void k_ovl_runs(const int32_t* __restrict__ raw, OvlFiles S,
                                                      const OvlTile* __restrict__ tiles, int min_steps,
                                                      int32_t* __restrict__ pair) {
    const OvlTile tl = tiles[blockIdx.x];
    const long long T = S.files[(long long)tl.file * TD_FILE + TDF_T];
    const long long t = (long long)tl.step0 + threadIdx.x;
    if (t >= T) return;
    const int32_t* r = raw + S.step_off[tl.file];
    const int32_t v = r[t];
    int32_t keep = -1;
    if (v != -1) {
        int run = 1;
        for (long long u = t - 1; u >= 0 && run < min_steps && r[u] == v; --u) ++run;
        for (long long u = t + 1; u < T && run < min_steps && r[u] == v; ++u) ++run;
        if (run >= min_steps) keep = v;
    }
    int32_t* o = pair + 2 * (S.step_off[tl.file] + t);
    o[0] = keep == -1 ? -1 : (keep & 0xff);
    o[1] = keep == -1 ? -1 : (keep >> 8);
}

}  // namespace spkd
