// The seed stage of the self-trained speech / non-speech detector (spkd_frame_energy_batch,
// spkd_energy_seeds): frame energies from the samples of a batch and, per file, two order statistics
// of them and the runs of frames at or beyond each.  Everything is integer arithmetic, so every value
// is exact and depends neither on the grid nor on the neighbouring files.
//
//   k_frame_energy : workgroup per tile of one file (a tile never crosses a file; the file is found by
//                    mf_file_of on the block index): the frames whose hops fill EN_TILE samples.  The
//                    tile's span, its frames' hops and the last frame's window, is cut into cells of 8
//                    samples on the 16-byte grid of the address space, so a cell inside the file is one
//                    16-byte load and neighbouring lanes take neighbouring cells; a cell that crosses
//                    the tile's start or the file's end is read sample by sample, zero outside.  Each
//                    sample is added once, into its cell's (sum s, sum s^2); the cells are scanned in
//                    LDS (a run of cells per thread, a wave scan, the waves' totals), and a frame is two
//                    look-ups: prefix(t hop + window) - prefix(t hop).  A frame border inside a cell adds
//                    the cell's samples in front of it again (at most 7, from L1 / L2); with the sample
//                    offsets, the hop and the window multiples of 8 there is none.  Of the overlap of two
//                    tiles, window - hop samples, the second read comes from L2.
//                    sum s wraps in 32 bits and sum s^2 in 64: a frame's own sums fit (|sum s| <= 2^27,
//                    sum s^2 <= 2^42), and a difference of wrapped prefixes is the wrapped difference.
//   k_energy_select: workgroup per file.  Eight passes over the file's energies, most significant byte
//                    first: a 256-bin histogram in LDS of the keys that share the bytes chosen so far,
//                    one for the k_low-th smallest and one for the k_high-th largest (as the
//                    (T - k_high + 1)-th smallest), both filled by the same pass.  Then the file's seeded
//                    flag and, for a seeded file, the number of runs of either class.
//   k_energy_runs  : workgroup per file, behind the host's prefix sum of those counts: a flag per frame
//                    and class for "a run starts here", a scan of the flags over the file (tile by tile
//                    with a carry), and the compaction: the j-th start and the j-th end of a class are
//                    one run, and the end at frame i is that of the last run started at or before i.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_mfcc_batch.hpp"

namespace spkd {

constexpr int EN_MAX_WINDOW = 4096;      // hop <= window <= this (SPKD_ENERGY_MAX_WINDOW)
constexpr int EN_TILE = 16384;           // samples whose hops make a workgroup's frames (SPKD_ENERGY_TILE)
constexpr int EN_TPB = 256;
constexpr int EN_CELL = 8;               // samples of a 16-byte load
// cells of a tile: up to 7 samples in front of it down to the 16-byte grid, its span of at most
// EN_TILE - hop + window samples, a last cell begun; and the entry behind the last cell for the total
constexpr int EN_MAX_CELLS = (EN_CELL - 1 + EN_TILE + EN_MAX_WINDOW + EN_CELL - 1) / EN_CELL + 1;
constexpr int EN_RUN = (EN_MAX_CELLS + EN_TPB - 1) / EN_TPB;     // cells a thread scans
static_assert(EN_MAX_CELLS * 12 <= 64 * 1024, "the cells' prefixes fit the static LDS of a workgroup");

// frames of a tile: those whose hops fit EN_TILE samples (at least 4: hop <= 4096)
__host__ __device__ constexpr long long en_tile_frames(int hop) { return EN_TILE / hop; }

// sample `at` of the file (0 outside it)
__device__ inline int en_sample(const int16_t* __restrict__ pcm, long long n_samples, long long at) {
    return at >= 0 && at < n_samples ? (int)pcm[at] : 0;
}

__global__ __launch_bounds__(EN_TPB) void k_frame_energy(
        const int16_t* __restrict__ pcm, const long long* __restrict__ sample_off, const long long* __restrict__ frame_off,
        const long long* __restrict__ tile_off /* [n_files + 1] each */, long long n_files, int hop, int window,
        long long* __restrict__ energy) {
    __shared__ unsigned long long p2[EN_MAX_CELLS];      // sum s^2 of a cell, then of all cells before it
    __shared__ unsigned int p1[EN_MAX_CELLS];            // sum s likewise (wrapping)
    __shared__ unsigned long long w2[EN_TPB / 64];
    __shared__ unsigned int w1[EN_TPB / 64];
    const int tid = threadIdx.x;
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const long long n_samples = sample_off[file + 1] - sample_off[file];
    const long long n_frames = frame_off[file + 1] - frame_off[file];
    const long long per_tile = en_tile_frames(hop);
    const long long t0 = ((long long)blockIdx.x - tile_off[file]) * per_tile;          // in the file
    const int cnt = (int)(n_frames - t0 < per_tile ? n_frames - t0 : per_tile);
    pcm += sample_off[file];
    energy += frame_off[file] + t0;
    const long long s0 = t0 * hop;                                                     // the tile's first sample
    // the span that holds a sample: the frames' hops and the last window, cut at the file's end
    long long span = (long long)(cnt - 1) * hop + window;
    if (span > n_samples - s0) span = n_samples - s0;
    const int lead = (int)(((unsigned long long)(pcm + s0) & 15ull) >> 1);             // samples down to the 16-byte grid
    const int n_cells = (lead + (int)span + EN_CELL - 1) / EN_CELL;                    // <= EN_MAX_CELLS - 1
    const int16_t* const grid0 = pcm + s0 - lead;                                      // cell 0 (16-byte aligned)
    for (int c = tid; c < n_cells; c += EN_TPB) {
        const int rel = c * EN_CELL - lead;                                            // of the cell's first sample, in the tile
        int s[EN_CELL];
        if (rel >= 0 && rel + EN_CELL <= span) {
            const int4 v = *(const int4*)(grid0 + c * EN_CELL);
            const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[2 * i] = (int)(short)(w[i] & 0xffff);
                s[2 * i + 1] = w[i] >> 16;
            }
        } else {
#pragma unroll
            for (int i = 0; i < EN_CELL; ++i) s[i] = rel + i >= 0 && rel + i < span ? (int)pcm[s0 + rel + i] : 0;
        }
        unsigned int a1 = 0;
        unsigned long long a2 = 0;
#pragma unroll
        for (int i = 0; i < EN_CELL; ++i) {
            a1 += (unsigned int)s[i];
            a2 += (unsigned long long)(s[i] * s[i]);                                   // (2^30 at most: -32768 squared)
        }
        p1[c] = a1;
        p2[c] = a2;
    }
    __syncthreads();
    // exclusive scan of the cells: a run of consecutive cells per thread, the threads by a wave scan,
    // the waves through LDS
    const int run = (n_cells + EN_TPB - 1) / EN_TPB;
    const int c0 = tid * run < n_cells ? tid * run : n_cells;
    const int c1 = c0 + run < n_cells ? c0 + run : n_cells;
    unsigned int m1 = 0;
    unsigned long long m2 = 0;
    for (int c = c0; c < c1; ++c) {
        m1 += p1[c];
        m2 += p2[c];
    }
    unsigned int i1 = m1;                                                              // inclusive over the threads
    unsigned long long i2 = m2;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned int u1 = __shfl_up(i1, d, 64);
        const unsigned long long u2 = __shfl_up(i2, d, 64);
        if (lane >= d) {
            i1 += u1;
            i2 += u2;
        }
    }
    if (lane == 63) {
        w1[wave] = i1;
        w2[wave] = i2;
    }
    __syncthreads();
    for (int v = 0; v < wave; ++v) {
        i1 += w1[v];
        i2 += w2[v];
    }
    unsigned int e1 = i1 - m1;                                                         // exclusive: all cells before c0
    unsigned long long e2 = i2 - m2;
    for (int c = c0; c < c1; ++c) {
        const unsigned int v1 = p1[c];
        const unsigned long long v2 = p2[c];
        p1[c] = e1;
        p2[c] = e2;
        e1 += v1;
        e2 += v2;
    }
    if (tid == EN_TPB - 1) {                                                           // the total, behind the last cell
        p1[n_cells] = i1;
        p2[n_cells] = i2;
    }
    __syncthreads();
    for (int f = tid; f < cnt; f += EN_TPB) {
        unsigned int q1[2];
        unsigned long long q2[2];
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            long long x = (long long)f * hop + (side ? window : 0);                    // sums of the samples before x
            if (x > span) x = span;
            const int pos = (int)x + lead, c = pos / EN_CELL, m = pos % EN_CELL;
            unsigned int a1 = p1[c];
            unsigned long long a2 = p2[c];
            for (int i = 0; i < m; ++i) {                                              // the cell's samples in front of x
                const int rel = c * EN_CELL - lead + i;
                const int v = rel >= 0 ? (int)pcm[s0 + rel] : 0;                       // (rel < x <= span: inside the file)
                a1 += (unsigned int)v;
                a2 += (unsigned long long)(v * v);
            }
            q1[side] = a1;
            q2[side] = a2;
        }
        const long long sum = (long long)(int)(q1[1] - q1[0]);
        const long long sq = (long long)(q2[1] - q2[0]);
        energy[f] = (long long)window * sq - sum * sum;
    }
}

// ---- the order statistics and the runs
constexpr int ES_TPB = 1024;
constexpr int ES_BINS = 256;
constexpr int ES_PASSES = 8;             // of 8 bits over the 64-bit key

struct EsFile {                          // what k_energy_select leaves per file
    long long lo, hi;
    long long n_runs[2];
    int seeded, pad;
};

__device__ inline bool es_in_class(long long e, int cls, long long lo, long long hi) { return cls ? e >= hi : e <= lo; }

// the sum over the workgroup of one value per thread, for every thread (two barriers)
__device__ inline long long es_block_sum(long long v, long long* __restrict__ waves /* [ES_TPB / 64] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();                                                                   // (the last use of waves[] is over)
    if (lane == 0) waves[wave] = v;
    __syncthreads();
    long long total = 0;
    for (int w = 0; w < ES_TPB / 64; ++w) total += waves[w];
    return total;
}

__global__ __launch_bounds__(ES_TPB) void k_energy_select(
        const long long* __restrict__ energy, const long long* __restrict__ frame_off, const long long* __restrict__ k_low,
        const long long* __restrict__ k_high /* [n_files] */, EsFile* __restrict__ out) {
    __shared__ unsigned int hist[2][ES_BINS];
    __shared__ unsigned long long prefix[2];             // the key's bytes chosen so far, in place
    __shared__ unsigned long long rank[2];               // 1-based, among the keys that share them
    __shared__ long long waves[ES_TPB / 64];
    const int tid = threadIdx.x;
    const long long file = blockIdx.x;
    const long long T = frame_off[file + 1] - frame_off[file];
    const unsigned long long* const key = (const unsigned long long*)energy + frame_off[file];   // (an energy is >= 0)
    const long long kl = k_low[file], kh = k_high[file];
    const bool valid = kl >= 1 && kh >= 1 && kl <= T && kh <= T;
    EsFile r = {0, 0, {0, 0}, 0, 0};
    if (valid) {                                                                       // (the same in every thread)
        if (tid < 2) {
            prefix[tid] = 0;
            rank[tid] = tid ? (unsigned long long)(T - kh + 1) : (unsigned long long)kl;
        }
        for (int pass = 0; pass < ES_PASSES; ++pass) {
            const int shift = 64 - 8 * (pass + 1);
            for (int b = tid; b < 2 * ES_BINS; b += ES_TPB) (&hist[0][0])[b] = 0;
            __syncthreads();
            // the bytes above this pass's: all keys share them in pass 0
            const unsigned long long mask = pass ? ~0ull << (shift + 8) : 0ull;
            const unsigned long long want0 = prefix[0], want1 = prefix[1];
            for (long long i = tid; i < T; i += ES_TPB) {
                const unsigned long long k = key[i];
                const unsigned int b = (unsigned int)(k >> shift) & (ES_BINS - 1);
                if ((k & mask) == want0) atomicAdd(&hist[0][b], 1u);
                if ((k & mask) == want1) atomicAdd(&hist[1][b], 1u);
            }
            __syncthreads();
            if (tid == 0 || tid == 64) {                                               // a wave each
                const int which = tid ? 1 : 0;
                unsigned long long left = rank[which];
                int b = 0;
                for (; b < ES_BINS - 1 && left > hist[which][b]; ++b) left -= hist[which][b];
                rank[which] = left;
                prefix[which] |= (unsigned long long)b << shift;
            }
            __syncthreads();
        }
        r.lo = (long long)prefix[0];
        r.hi = (long long)prefix[1];
        r.seeded = r.lo < r.hi;
    }
    if (r.seeded) {
        long long starts[2] = {0, 0};
        for (long long i = tid; i < T; i += ES_TPB) {
            const long long e = energy[frame_off[file] + i];
            const long long before = i > 0 ? energy[frame_off[file] + i - 1] : 0;
#pragma unroll
            for (int cls = 0; cls < 2; ++cls)
                starts[cls] += es_in_class(e, cls, r.lo, r.hi) && (i == 0 || !es_in_class(before, cls, r.lo, r.hi));
        }
        r.n_runs[0] = es_block_sum(starts[0], waves);
        r.n_runs[1] = es_block_sum(starts[1], waves);
    }
    if (tid == 0) out[file] = r;
}

__global__ __launch_bounds__(ES_TPB) void k_energy_runs(
        const long long* __restrict__ energy, const long long* __restrict__ frame_off, const EsFile* __restrict__ files,
        const long long* __restrict__ run_off /* [2 n_files + 1] */, long long* __restrict__ run_begin,
        long long* __restrict__ run_end) {
    __shared__ unsigned long long waves[ES_TPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long file = blockIdx.x;
    const EsFile r = files[file];
    if (!r.seeded) return;
    const long long first = frame_off[file], T = frame_off[file + 1] - first;
    energy += first;
    // both classes' counts of starts in one word: class 0 low, class 1 high (a file has fewer than 2^32 frames)
    unsigned long long carry = 0;
    for (long long base = 0; base < T; base += ES_TPB) {
        const long long i = base + tid;
        bool in[2] = {false, false}, start[2] = {false, false}, end[2] = {false, false};
        if (i < T) {
            const long long e = energy[i];
            const long long before = i > 0 ? energy[i - 1] : 0, after = i + 1 < T ? energy[i + 1] : 0;
#pragma unroll
            for (int cls = 0; cls < 2; ++cls) {
                in[cls] = es_in_class(e, cls, r.lo, r.hi);
                start[cls] = in[cls] && (i == 0 || !es_in_class(before, cls, r.lo, r.hi));
                end[cls] = in[cls] && (i + 1 == T || !es_in_class(after, cls, r.lo, r.hi));
            }
        }
        unsigned long long inc = (unsigned long long)start[0] | ((unsigned long long)start[1] << 32);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long u = __shfl_up(inc, d, 64);
            if (lane >= d) inc += u;
        }
        __syncthreads();                                                               // (the tile before has read waves[])
        if (lane == 63) waves[wave] = inc;
        __syncthreads();
        unsigned long long total = 0;
        for (int w = 0; w < ES_TPB / 64; ++w) {
            if (w < wave) inc += waves[w];
            total += waves[w];
        }
        inc += carry;                                                                  // starts at or before frame i
        carry += total;
#pragma unroll
        for (int cls = 0; cls < 2; ++cls) {
            const long long n = (long long)((inc >> (32 * cls)) & 0xffffffffull);
            const long long slot = run_off[2 * file + cls] + n - 1;                    // of the last run started
            if (start[cls]) run_begin[slot] = first + i;
            if (end[cls]) run_end[slot] = first + i + 1;
        }
    }
}

}  // namespace spkd
