// Feature warping ahead of linking by cross-likelihood ratio (spkd_feature_warp): over a sliding window of a
// file's speech every coefficient becomes the standard-normal quantile of its rank in the window.  The rule
// is include/spkd.h, section 10b; nothing of it is restated here beyond what the code does.
// PARITY: no reference counterpart -- the reference links nothing across files; tests/warp_numpy.py restates
// the rule frame by frame.
//
//   k_feature_warp : one workgroup per tile of WP_TILE compacted frames of one set (the tile table is the
//                    host's).  Phase 1, a thread per frame of the tile and its halo (at most WP_TILE + n - 1):
//                    the frame's place in the batch through the set's run table.  Phase 2: those frames into
//                    LDS as keys (wp_key), dimension-major, so that lanes that own neighbouring frames of one
//                    dimension read neighbouring banks.  Phase 3, a wave per (dimension, 64 lanes): a lane owns
//                    WP_R consecutive frames and reads the union of their windows once; only the WP_R - 1
//                    entries at either edge are predicated.  WP_R is odd, so the lanes' stride has no bank
//                    conflict.  The results wait in registers until every wave has counted, replace the
//                    tile's keys in LDS and go out frame-major, whole rows.
// The counts without a compare.  2 lt + eq = lt + le, and a window entry x adds (x < v) + (x <= v) =
// 1 + sgn(v - x) to that; a NaN entry is to add 0.  So the frames become integer keys in the order of their
// values -- -0.0 the key of 0.0, a NaN the largest key, above +inf's, so that sgn(v - x) = -1 for it -- and
// the table index 2 lt + eq - 1 is n - 1 + sum sgn(key(v) - key(x)) over all n entries: a saturating
// subtraction, a clamp to [-1, 1] and an addition per entry, no condition mask.
// Integer arithmetic and one look-up in the caller's table: the bits depend neither on the run nor on the tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_device.hpp"

namespace spkd {

constexpr int WP_MAX_WINDOW = 512;    // the widest window (SPKD_WARP_MAX_WINDOW)
constexpr int WP_TILE = 384;          // compacted frames per workgroup (SPKD_WARP_TILE)
#ifndef SPKD_WARP_R
#define SPKD_WARP_R 3                 // (1: the plain count loop, a frame a lane -- for A/B builds)
#endif
constexpr int WP_R = SPKD_WARP_R;     // frames a lane owns
constexpr int WP_TPB = 1024;
constexpr int WP_WAVES = WP_TPB / WAVE;
constexpr int WP_GROUPS = WP_TILE / (WP_R * WAVE);                  // waves' worth of lanes per dimension
constexpr int WP_TASKS = D * WP_GROUPS;                             // (dimension, group) pairs of a tile
constexpr int WP_PER_WAVE = (WP_TASKS + WP_WAVES - 1) / WP_WAVES;   // of which a wave takes at most these
constexpr int WP_UNROLL = 8;                                        // window entries per trip of the count loop
static_assert(WP_R % 2 == 1 && WP_TILE % (WP_R * WAVE) == 0, "an odd stride, whole waves per dimension");

// the LDS of a launch whose widest window is n: the places of a tile's frames and its halo's, WP_TILE + n - 1
// of them, then their keys (an odd row stride: phase 2 writes a frame's 39 keys a stride apart)
__host__ __device__ constexpr int wp_stride(int n) { return (WP_TILE + n - 1) | 1; }
__host__ __device__ constexpr size_t wp_lds_bytes(int n) {
    return (size_t)(WP_TILE + n - 1) * sizeof(long long) + (size_t)D * wp_stride(n) * sizeof(float);
}
constexpr size_t WP_LDS_MAX = wp_lds_bytes(WP_MAX_WINDOW);
static_assert(WP_LDS_MAX <= 160 * 1024, "the widest window's tile fits a CU's LDS");

// The key of a value: signed integers in the order of the floats, key(-0.0) = key(0.0) = 0, key(NaN) = the
// largest int (the bit patterns above +inf's are NaNs, so no number has it).
constexpr int WP_NAN_KEY = 0x7fffffff;
__device__ __forceinline__ int wp_key(float x) {
    int b = __float_as_int(x);
    if (x != x) return WP_NAN_KEY;
    if (b == (int)0x80000000) b = 0;
    return b ^ ((b >> 31) & 0x7fffffff);
}
// sgn(v - x) of two keys, whose difference may leave 32 bits
__device__ __forceinline__ int wp_sgn(int v, int x) {
    const int d = __builtin_elementwise_sub_sat(v, x);
    // the clamp to [-1, 1] as the one instruction it is (written as min / max the compiler sees a three-way
    // compare in it and emits two compares and two selects)
    int s;
    asm("v_med3_i32 %0, %1, -1, 1" : "=v"(s) : "v"(d));
    return s;
}

// lo of frame j of a set of L frames under a window of n <= L (include/spkd.h, section 10b)
__device__ __forceinline__ long long wp_lo(long long j, int n, long long L) {
    const long long lo = j - n / 2;
    return lo < 0 ? 0 : lo > L - n ? L - n : lo;
}

__global__ __launch_bounds__(WP_TPB) void k_feature_warp(
        const float* __restrict__ frames, const long long* __restrict__ run_begin, const long long* __restrict__ run_ord,
        const long long* __restrict__ set_off, const long long* __restrict__ set_len,
        const long long* __restrict__ table_off, const float* __restrict__ table, const int* __restrict__ tile_set,
        const int* __restrict__ tile_idx, int window, int n_max, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char wp_lds[];
    long long* fr = (long long*)wp_lds;                                 // [WP_TILE + n_max - 1]
    int* xs = (int*)(wp_lds + (size_t)(WP_TILE + n_max - 1) * sizeof(long long));     // keys, then the tile's results' bits
    const int S = wp_stride(n_max);
    const int tid = threadIdx.x;
    const int s = tile_set[blockIdx.x];
    const long long L = set_len[s];
    const int n = window < L ? window : (int)L;
    const long long j0 = (long long)tile_idx[blockIdx.x] * WP_TILE;
    const int nt = L - j0 < WP_TILE ? (int)(L - j0) : WP_TILE;          // (>= 1: the host makes no empty tile)
    const long long s0 = wp_lo(j0, n, L);
    const int span = (int)(wp_lo(j0 + nt - 1, n, L) + n - s0);          // <= nt + n - 1
    const int own = (int)(j0 - s0);                                     // the tile's first frame within the span

    // phase 1: the run of every compacted frame of the span -- the last one that starts at or before it
    // (an empty run shares its ordinal with the next one, which wins)
    const long long r0 = set_off[s], r1 = set_off[s + 1];
    for (int i = tid; i < span; i += WP_TPB) {
        const long long e = s0 + i;
        long long a = r0, b = r1;                                       // run_ord[a] <= e < run_ord[b] (r1: L)
        while (b - a > 1) {
            const long long m = (a + b) >> 1;
            if (run_ord[m] <= e) a = m; else b = m;
        }
        fr[i] = run_begin[a] + (e - run_ord[a]);
    }
    __syncthreads();
    // phase 2: rows in, dimension-major, as keys
    for (int idx = tid; idx < span * D; idx += WP_TPB) {
        const int i = idx / D, d = idx - i * D;
        xs[d * S + i] = wp_key(frames[fr[i] * D + d]);
    }
    __syncthreads();

    // phase 3: the counts
    const int wave = tid / WAVE, lane = tid % WAVE;
    const float* __restrict__ tab = table + table_off[s];
    float res[WP_PER_WAVE][WP_R];
#pragma unroll
    for (int k = 0; k < WP_PER_WAVE; ++k) {
        const int task = wave + k * WP_WAVES;
        if (task >= WP_TASKS) break;                                    // (wave-uniform)
        const int d = task / WP_GROUPS;
        const int first = ((task - d * WP_GROUPS) * WAVE + lane) * WP_R;    // the lane's first frame within the tile
        const int* __restrict__ col = xs + d * S;
        int lo[WP_R], sg[WP_R], v[WP_R];
#pragma unroll
        for (int r = 0; r < WP_R; ++r) {
            // a frame past the tile's end repeats the tile's last one: its counts are not kept
            const int t = first + r < nt ? first + r : nt - 1;
            lo[r] = (int)(wp_lo(j0 + t, n, L) - s0);
            v[r] = col[own + t];
            sg[r] = 0;
        }
        // the union of the windows [lo[0], lo[WP_R - 1] + n): what every window holds in the middle, and at
        // most WP_R - 1 entries before and behind it that some hold
        const int mid0 = lo[WP_R - 1];
        const int mid1 = lo[0] + n > mid0 ? lo[0] + n : mid0;
        auto edge = [&](int e) {
            const int x = col[e];
#pragma unroll
            for (int r = 0; r < WP_R; ++r) sg[r] += e >= lo[r] && e < lo[r] + n ? wp_sgn(v[r], x) : 0;
        };
        for (int e = lo[0]; e < mid0; ++e) edge(e);
        // (unrolled by hand: the compiler leaves a loop around wp_sgn's instruction as it is)
        int e = mid0;
        for (; e + WP_UNROLL <= mid1; e += WP_UNROLL) {
            int x[WP_UNROLL];
#pragma unroll
            for (int u = 0; u < WP_UNROLL; ++u) x[u] = col[e + u];
#pragma unroll
            for (int r = 0; r < WP_R; ++r)
#pragma unroll
                for (int u = 0; u < WP_UNROLL; u += 2) sg[r] += wp_sgn(v[r], x[u]) + wp_sgn(v[r], x[u + 1]);
        }
        for (; e < mid1; ++e) {
            const int x = col[e];
#pragma unroll
            for (int r = 0; r < WP_R; ++r) sg[r] += wp_sgn(v[r], x);
        }
        for (int e = mid1; e < mid0 + n; ++e) edge(e);
#pragma unroll
        for (int r = 0; r < WP_R; ++r) {
            int at = n - 1 + sg[r];                                     // 2 lt + eq - 1, in [0, 2 n - 2] unless v is a NaN
            at = at < 0 ? 0 : at > 2 * n - 2 ? 2 * n - 2 : at;
            res[k][r] = v[r] == WP_NAN_KEY ? __int_as_float(0x7fc00000) : tab[at];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < WP_PER_WAVE; ++k) {
        const int task = wave + k * WP_WAVES;
        if (task >= WP_TASKS) break;
        const int d = task / WP_GROUPS;
        const int first = ((task - d * WP_GROUPS) * WAVE + lane) * WP_R;
#pragma unroll
        for (int r = 0; r < WP_R; ++r)
            if (first + r < nt) xs[d * S + own + first + r] = __float_as_int(res[k][r]);
    }
    __syncthreads();
    // rows out: the tile's frames only
    for (int idx = tid; idx < nt * D; idx += WP_TPB) {
        const int i = idx / D, d = idx - i * D;
        out[fr[own + i] * D + d] = __int_as_float(xs[d * S + own + i]);
    }
}

}  // namespace spkd
