// K_stats: frames -> packed sufficient-statistics records.
//
// Replaces the inputs of every np.cov call of the clustering scripts
// (get_spk_features + np.cov, spk-clustering.py:46-52,88-94): instead of copying
// and re-scanning raw frames per distance, each frame is read ONCE and folded
// into the augmented second-moment record of its set.
//
// Two deterministic passes (no float atomics, so results are bit-reproducible):
//   k_chunk_stats : one workgroup per chunk of <= STATS_CHUNK consecutive frames
//                   of one range; frames staged through LDS (converted to fp64
//                   once), 4 x 4 register-blocked fp64 accumulation per lane;
//   k_reduce_sets : per set, sums its chunk partials in chunk order.
// Algorithmic bytes: 156 B per frame read + 6 560 B per set written.
#pragma once
#include "spkd_device.hpp"

namespace spkd {

struct Chunk {
    int64_t begin;      // first frame
    int32_t len;        // frames in the chunk
    int32_t set;        // owning set
};

constexpr int STATS_TPB = 256;
constexpr int STATS_WAVES = STATS_TPB / WAVE;
constexpr int STATS_TILE = 64;        // frames staged per LDS tile
constexpr int STATS_CHUNK = 1024;     // frames per chunk (host splits ranges)
constexpr int SB = 4;                 // register block: each lane owns a 4 x 4 block of entries
constexpr int SNB = DA / SB;          // 10 block rows / columns
constexpr int SBLOCKS = SNB * (SNB + 1) / 2;   // 55 upper-triangular blocks per wave
constexpr int STATS_ENTRIES = (REC + STATS_TPB - 1) / STATS_TPB;   // record entries per thread

// Register-blocked accumulation: a wave covers the whole 40 x 40 upper triangle with
// 55 lanes, each holding a 4 x 4 block of fp64 accumulators; per frame a lane reads
// 4 + 4 doubles from the LDS tile (two ds_read_b128 pairs, broadcast among the lanes
// that share a block row / column) and issues 16 FMAs -- 1.5 instructions per entry
// instead of 5 for the one-entry-per-thread form.  The four waves of the workgroup
// take every fourth frame of the tile; their partial blocks are summed through LDS
// in wave order at the end (deterministic).
//
// The body, for the workgroup's STATS_TPB threads: the moment sums of the `len` >= 1 frames from
// `begin` on; thread tid gets entry e = tid + k * STATS_TPB of the packed record as emit(k, e, v),
// k < STATS_ENTRIES.  xs / part: the workgroup's LDS; a second call may follow behind a barrier.
//
// wt weighs the frames (spkd_post_stats.hpp); UnitWeight, an empty object, is weight 1 for all:
//   wt.issue(t0, tl)   with the tile's global loads: fetch the weights of the tl frames from t0 on;
//   wt.stage()         with the tile's LDS stores, ahead of the barrier: hand them to the workgroup;
//   wt.skip(f)         frame f of the staged tile takes no part (asked before its values are read);
//   wt.scale(f, xi)    xi *= w_f, ahead of the 16 FMAs.
struct UnitWeight {
    __device__ __forceinline__ void issue(int, int) {}
    __device__ __forceinline__ void stage() {}
    __device__ __forceinline__ bool skip(int) const { return false; }
    __device__ __forceinline__ void scale(int, double (&)[SB]) const {}
};

template <class Emit, class Weight = UnitWeight>
__device__ __forceinline__ void chunk_stats_accumulate(
        const float* __restrict__ frames, int64_t begin, int len,
        double (&xs)[STATS_TILE][DA], double (&part)[STATS_WAVES][SBLOCKS][SB * SB], Emit emit, Weight wt = Weight()) {
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    // lane -> block (bi <= bj)
    int bi = 0, rem = lane < SBLOCKS ? lane : 0;
    while (rem >= SNB - bi) { rem -= SNB - bi; ++bi; }
    const int bj = bi + rem;
    double acc[SB][SB];
#pragma unroll
    for (int a = 0; a < SB; ++a)
#pragma unroll
        for (int b = 0; b < SB; ++b) acc[a][b] = 0.0;
    const float* base = frames + begin * (int64_t)D;
    // software pipeline: the floats of tile k+1 are loaded into registers while tile k
    // is being accumulated, so the global latency is paid once per chunk, not per tile
    constexpr int PF = (STATS_TILE * D + STATS_TPB - 1) / STATS_TPB;      // 10 floats per thread
    int loff[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
        const int idx = tid + STATS_TPB * k;
        const int f = idx / D;
        loff[k] = f * DA + (idx - f * D);
    }
    float pf[PF];
    auto issue = [&](int t0) {
        const int tl = min(STATS_TILE, len - t0);
        const float* src = base + (int64_t)t0 * D;
#pragma unroll
        for (int k = 0; k < PF; ++k) {
            const int idx = tid + STATS_TPB * k;
            pf[k] = idx < tl * D ? src[idx] : 0.0f;
        }
        wt.issue(t0, tl);
    };
    issue(0);
    double* xsf = &xs[0][0];
    for (int t0 = 0; t0 < len; t0 += STATS_TILE) {
        const int tl = min(STATS_TILE, len - t0);
#pragma unroll
        for (int k = 0; k < PF; ++k)
            if (tid + STATS_TPB * k < STATS_TILE * D) xsf[loff[k]] = (double)pf[k];
        if (tid < STATS_TILE) xs[tid][D] = 1.0;
        wt.stage();
        __syncthreads();
        if (t0 + STATS_TILE < len) issue(t0 + STATS_TILE);
        for (int f = wave; f < tl; f += STATS_WAVES) {
            if (wt.skip(f)) continue;
            double xi[SB], xj[SB];
#pragma unroll
            for (int a = 0; a < SB; ++a) { xi[a] = xs[f][SB * bi + a]; xj[a] = xs[f][SB * bj + a]; }
            wt.scale(f, xi);
#pragma unroll
            for (int a = 0; a < SB; ++a)
#pragma unroll
                for (int b = 0; b < SB; ++b) acc[a][b] = fma(xi[a], xj[b], acc[a][b]);
        }
        __syncthreads();
    }
    if (lane < SBLOCKS) {
#pragma unroll
        for (int a = 0; a < SB; ++a)
#pragma unroll
            for (int b = 0; b < SB; ++b) part[wave][lane][a * SB + b] = acc[a][b];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < STATS_ENTRIES; ++k) {
        const int e = tid + k * STATS_TPB;
        if (e < REC) {
            int r, c;
            decode_entry(e, r, c);
            const int pbi = r / SB, pbj = c / SB;
            const int blk = pbi * SNB - (pbi * (pbi - 1)) / 2 + (pbj - pbi);
            const int w = (r % SB) * SB + (c % SB);
            double v = part[0][blk][w];
#pragma unroll
            for (int q = 1; q < STATS_WAVES; ++q) v += part[q][blk][w];
            emit(k, e, v);
        }
    }
}

__global__ __launch_bounds__(STATS_TPB) void k_chunk_stats(
        const float* __restrict__ frames, const Chunk* __restrict__ chunks,
        double* __restrict__ partial) {
    __shared__ double xs[STATS_TILE][DA];                       // 20 KB
    __shared__ double part[STATS_WAVES][SBLOCKS][SB * SB];      // 28 KB
    const Chunk ch = chunks[blockIdx.x];
    double* out = partial + (int64_t)blockIdx.x * REC;
    chunk_stats_accumulate(frames, ch.begin, ch.len, xs, part, [&](int, int e, double v) { out[e] = v; });
}

// set s owns chunks [set_chunk_off[s], set_chunk_off[s+1])
__global__ __launch_bounds__(STATS_TPB) void k_reduce_sets(
        const double* __restrict__ partial, const int64_t* __restrict__ set_chunk_off,
        double* __restrict__ stats) {
    const int64_t s = blockIdx.x;
    const int64_t c0 = set_chunk_off[s], c1 = set_chunk_off[s + 1];
    for (int e = threadIdx.x; e < REC; e += STATS_TPB) {
        double acc = 0.0;
        for (int64_t c = c0; c < c1; ++c) acc += partial[c * REC + e];
        stats[s * REC + e] = acc;
    }
}

// K_sum: records -> sums of records (spkd_sum_stats).  A record is a raw moment sum, so the
// record of a union of frame sets is the sum of their records: set s owns the members
// member[set_off[s] .. set_off[s+1]), indices into src, and dst[s] is their entry-wise sum in
// member order -- the first member copied, every later one added to it, one chain of fp64
// additions per entry (no atomics, no tree: the bits are those of a host loop in that order).
// One workgroup per set; a record is 410 double2, and thread t < 205 owns the two at t and
// t + 205 of every record (a wave reads 1 KiB of a record at a stretch; the other 51 threads of
// the workgroup leave at once: there is no barrier).  The members go by in batches of SUM_DEPTH
// in two register sets that take turns: the loads of a batch are all issued before the batch
// ahead of it is added, so the waits are counted ones and 8 to 16 loads a thread are in flight.
// A streaming kernel: members x 6 560 B read, sets x 6 560 B written.
constexpr int SUM_TPB = 256;
constexpr int SUM_OWN = 2;                                        // double2 per active thread
constexpr int SUM_LANES = REC / 2 / SUM_OWN;                      // 205 active threads
constexpr int SUM_DEPTH = 4;                                      // members per batch
static_assert(SUM_LANES * SUM_OWN * 2 == REC && SUM_LANES <= SUM_TPB, "a record is 205 x 2 double2");

__global__ __launch_bounds__(SUM_TPB) void k_sum_records(
        const double* __restrict__ src, const int64_t* __restrict__ member,
        const int64_t* __restrict__ set_off, double* __restrict__ dst) {
    const int tid = threadIdx.x;
    if (tid >= SUM_LANES) return;
    const int64_t s = blockIdx.x;
    const int64_t m0 = set_off[s], m1 = set_off[s + 1];
    auto load = [&](int64_t m, double2 (&v)[SUM_OWN]) {
        const double2* r = reinterpret_cast<const double2*>(src + member[m] * REC);
#pragma unroll
        for (int k = 0; k < SUM_OWN; ++k) v[k] = r[tid + k * SUM_LANES];
    };
    auto fetch = [&](int64_t m, double2 (&buf)[SUM_DEPTH][SUM_OWN]) {
#pragma unroll
        for (int j = 0; j < SUM_DEPTH; ++j) load(m + j, buf[j]);
    };
    double2 acc[SUM_OWN];
    auto add = [&](const double2 (&v)[SUM_OWN]) {
#pragma unroll
        for (int k = 0; k < SUM_OWN; ++k) {
            acc[k].x += v[k].x;
            acc[k].y += v[k].y;
        }
    };
    auto add_batch = [&](const double2 (&buf)[SUM_DEPTH][SUM_OWN]) {
#pragma unroll
        for (int j = 0; j < SUM_DEPTH; ++j) add(buf[j]);
    };
    load(m0, acc);
    int64_t m = m0 + 1;
    const int64_t full = (m1 - m) / SUM_DEPTH;                   // whole batches behind the first member
    if (full > 0) {
        double2 a[SUM_DEPTH][SUM_OWN], b[SUM_DEPTH][SUM_OWN];
        fetch(m, a);
        int64_t k = 1;
        for (; k + 1 < full; k += 2) {
            fetch(m + k * SUM_DEPTH, b);
            add_batch(a);
            fetch(m + (k + 1) * SUM_DEPTH, a);
            add_batch(b);
        }
        if (k < full) {
            fetch(m + k * SUM_DEPTH, b);
            add_batch(a);
            add_batch(b);
        } else {
            add_batch(a);
        }
        m += full * SUM_DEPTH;
    }
    for (; m < m1; ++m) {                                        // fewer than SUM_DEPTH are left
        double2 v[SUM_OWN];
        load(m, v);
        add(v);
    }
    double2* d = reinterpret_cast<double2*>(dst + s * REC);
#pragma unroll
    for (int k = 0; k < SUM_OWN; ++k) d[tid + k * SUM_LANES] = acc[k];
}

}  // namespace spkd
