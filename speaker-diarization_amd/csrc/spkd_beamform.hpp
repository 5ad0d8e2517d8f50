// Delay-and-sum beamforming of a batch's multi-channel audio (spkd_bf_gcc, spkd_bf_track, spkd_bf_sum;
// include/spkd.h (6b2) has the definitions): per analysis step the GCC-PHAT correlation of every channel
// against a reference channel and its best lags, a Viterbi over the steps that picks one lag per step and
// channel, and the sum of the channels at those lags, cross-faded between steps.  PARITY UNPINNED: no
// reference counterpart (BeamformIt is the usual name of the scheme; it is not available and not
// restated); tests/beamform_numpy.py restates the three stages.
//
//   k_bf_twiddle : once per context, w[k] = e^{-2 pi i k / N} for k < N / 2, by the device's fp64 cospi /
//                  sinpi, rounded to float32 (no float32 recurrence).
//   k_bf_energy  : workgroup per BF_EN_TILE frames of one file (mf_file_of on the block index): per channel
//                  the sum of squares, reduced in the wave and added to the file's int64 word by an integer
//                  atomic -- exact, so the order of the additions does not matter.
//   k_bf_ref     : thread per file: the requested reference channel, or the arg-max of the energies (ties to
//                  the lowest index).
//   k_bf_gcc     : workgroup per (file, step, channel), 8 waves.  The reference window goes to the real
//                  parts and the channel's window to the imaginary parts of ONE 8192-point forward transform
//                  in LDS (float2, one pad element per 32 against the power-of-two strides: a bank row holds
//                  32 float2); the two spectra are separated by conjugate symmetry, G = P / |P| is written
//                  back Hermitian, and one inverse transform gives the real correlation.  The forward
//                  transform is decimation in frequency (natural order in, bit-reversed out), the inverse
//                  decimation in time (bit-reversed in, natural out), so nothing is ever permuted; G is formed
//                  on the bit-reversed image.  A pass does 3 or 4 radix-2 stages on 8 or 16 elements in
//                  registers (13 = 4 + 3 + 3 + 3).  A window that is all zero is detected on the integers: its
//                  spectrum is exactly 0, which float32 rounding of the packed transform would not keep.
//                  The selection over the 2 D + 1 lags follows in the same workgroup: four rounds of one
//                  block-wide arg-max, each over the candidates ranked behind the previous winner.
//                  The packing costs accuracy where a channel is much quieter than the reference: the
//                  separation subtracts two roundings of the louder spectrum (about 1e-7 of it).
//   k_bf_track   : thread per (file, channel), serial over the steps: four scores in fp64 (__dmul_rn /
//                  __dsub_rn / __dadd_rn: no contraction), one byte of four 2-bit back-pointers per step.
//                  The step a step takes its lags from waits in the delay array until the backtrack
//                  replaces it by the lag.
//   k_bf_sum     : workgroup per BF_SUM_TILE output samples of one file; the numerator is exact in int64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_mfcc_batch.hpp"

namespace spkd {

constexpr int BF_N = 8192;               // SPKD_BF_NFFT
constexpr int BF_LOG_N = 13;
constexpr int BF_NBEST = 4;              // SPKD_BF_NBEST
constexpr int BF_MAX_HOP = 1 << 20;      // SPKD_BF_MAX_HOP
constexpr int BF_MAX_CH = 8;             // (the resampler's limit: SPKD_RESAMPLE_MAX_CH)
constexpr int BF_TPB = 512;
constexpr int BF_PAD_LEN = BF_N + BF_N / 32;
constexpr int BF_LDS_BYTES = BF_PAD_LEN * 8;      // 67 584: two workgroups share a CU's 160 KiB
constexpr int BF_EN_TILE = 16384;        // frames per workgroup of k_bf_energy
constexpr int BF_EN_TPB = 256;
constexpr int BF_SUM_TILE = 2048;        // output samples per workgroup of k_bf_sum
constexpr int BF_SUM_TPB = 256;
static_assert(BF_N == 1 << BF_LOG_N, "the transform length");

struct BfGeom { int hop, window, max_lag; };

// steps of a file of n frames (C = 1: none, the file is copied through)
__host__ __device__ inline long long bf_steps(long long n, int C, int hop, int window) {
    if (C == 1) return 0;
    return n <= window ? 1 : (n - window) / hop + 1;
}

__device__ inline int bf_pad(int i) { return i + (i >> 5); }

__global__ void k_bf_twiddle(float2* __restrict__ tw /* [BF_N / 2] */) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= BF_N / 2) return;
    const double x = 2.0 * (double)k / (double)BF_N;
    tw[k] = make_float2((float)cospi(x), (float)-sinpi(x));
}

__global__ __launch_bounds__(BF_EN_TPB) void k_bf_energy(
        const int16_t* __restrict__ in, const long long* __restrict__ in_off, const long long* __restrict__ tile_off,
        long long n_files, const int* __restrict__ channels, unsigned long long* __restrict__ energy /* [n_files][8], zeroed */) {
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const int C = channels[file];
    const long long n = (in_off[file + 1] - in_off[file]) / C;
    const long long f0 = ((long long)blockIdx.x - tile_off[file]) * BF_EN_TILE;
    const long long f1 = f0 + BF_EN_TILE < n ? f0 + BF_EN_TILE : n;
    in += in_off[file];
    for (int c = 0; c < C; ++c) {
        unsigned long long s = 0;
        for (long long f = f0 + threadIdx.x; f < f1; f += BF_EN_TPB) {
            const long long v = in[f * C + c];
            s += (unsigned long long)(v * v);
        }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0 && s) atomicAdd(&energy[file * BF_MAX_CH + c], s);
    }
}

__global__ void k_bf_ref(const unsigned long long* __restrict__ energy, const int* __restrict__ channels,
                         const int* __restrict__ want, long long n_files, int* __restrict__ ref) {
    const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_files) return;
    int r = want[f];
    if (r < 0) {
        r = 0;
        for (int c = 1; c < channels[f]; ++c)
            if (energy[f * BF_MAX_CH + c] > energy[f * BF_MAX_CH + r]) r = c;
    }
    ref[f] = r;
}

__device__ inline float2 bf_cmul(float2 a, float2 w) { return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// K radix-2 stages on 2^K elements S apart, in registers.  Forward: the DIF stages of half sizes
// 2^(K-1) S .. S, twiddle w^(j N / 2h) behind the difference; inverse: the DIT stages S .. 2^(K-1) S, the
// conjugate twiddle in front of the butterfly.
template <int K, int S, bool INV>
__device__ inline void bf_pass(float2* __restrict__ z, const float2* __restrict__ tw, int tid) {
    constexpr int R = 1 << K;
    for (int t = tid; t < (BF_N >> K); t += BF_TPB) {
        const int low = t & (S - 1);
        const int base = (t / S) * (S << K) + low;
        float2 e[R];
#pragma unroll
        for (int r = 0; r < R; ++r) e[r] = z[bf_pad(base + r * S)];
        if (!INV) {
#pragma unroll
            for (int hr = R / 2; hr >= 1; hr >>= 1) {
                const int q = BF_N / (2 * hr * S);
#pragma unroll
                for (int blk = 0; blk < R; blk += 2 * hr)
#pragma unroll
                    for (int jr = 0; jr < hr; ++jr) {
                        const float2 a = e[blk + jr], b = e[blk + jr + hr];
                        e[blk + jr] = make_float2(a.x + b.x, a.y + b.y);
                        e[blk + jr + hr] = bf_cmul(make_float2(a.x - b.x, a.y - b.y), tw[(jr * S + low) * q]);
                    }
            }
        } else {
#pragma unroll
            for (int hr = 1; hr <= R / 2; hr <<= 1) {
                const int q = BF_N / (2 * hr * S);
#pragma unroll
                for (int blk = 0; blk < R; blk += 2 * hr)
#pragma unroll
                    for (int jr = 0; jr < hr; ++jr) {
                        const float2 w = tw[(jr * S + low) * q];
                        const float2 a = e[blk + jr], b = bf_cmul(e[blk + jr + hr], make_float2(w.x, -w.y));
                        e[blk + jr] = make_float2(a.x + b.x, a.y + b.y);
                        e[blk + jr + hr] = make_float2(a.x - b.x, a.y - b.y);
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) z[bf_pad(base + r * S)] = e[r];
    }
}

__device__ inline int bf_brev(int k) { return (int)(__brev((unsigned)k) >> (32 - BF_LOG_N)); }

// a ranks before b: the larger value, then the lower lag
__device__ inline bool bf_before(float av, int al, float bv, int bl) { return av > bv || (av == bv && al < bl); }

__global__ __launch_bounds__(BF_TPB) void k_bf_gcc(
        const int16_t* __restrict__ in, const long long* __restrict__ in_off, const long long* __restrict__ wg_off /* sum of T C */,
        long long n_files, const int* __restrict__ channels, const int* __restrict__ geom_of, const BfGeom* __restrict__ geoms,
        const int* __restrict__ ref_of, const float2* __restrict__ tw, int* __restrict__ lag_out, float* __restrict__ val_out,
        float* __restrict__ curve /* or null */, const long long* __restrict__ curve_off) {
    extern __shared__ __attribute__((aligned(16))) char bf_lds[];
    __shared__ float red_v[BF_TPB];
    __shared__ int red_l[BF_TPB];
    float2* z = (float2*)bf_lds;
    const int tid = threadIdx.x;
    const long long file = mf_file_of(wg_off, n_files, blockIdx.x);
    const int C = channels[file];
    const BfGeom g = geoms[geom_of[file]];
    const long long n = (in_off[file + 1] - in_off[file]) / C;
    const long long at = (long long)blockIdx.x - wg_off[file];
    const long long step = at / C;
    const int ch = (int)(at - step * C);
    const int ref = ref_of[file];
    const int D = g.max_lag, n_lag = 2 * D + 1;
    int* lag = lag_out + (long long)blockIdx.x * BF_NBEST;
    float* val = val_out + (long long)blockIdx.x * BF_NBEST;
    float* cv = curve ? curve + curve_off[file] + at * n_lag : nullptr;
    if (ch == ref) {                                   // by definition: lag 0 with value 1, and nothing else
        if (tid < BF_NBEST) { lag[tid] = 0; val[tid] = tid == 0 ? 1.0f : -INFINITY; }
        if (cv) for (int i = tid; i < n_lag; i += BF_TPB) cv[i] = i == D ? 1.0f : 0.0f;
        return;
    }
    in += in_off[file];
    const long long first = step * g.hop;
    int any_a = 0, any_b = 0;
    for (int i = tid; i < BF_N; i += BF_TPB) {
        const long long f = first + i;
        int a = 0, b = 0;
        if (i < g.window && f < n) { a = in[f * C + ref]; b = in[f * C + ch]; }
        any_a |= a;
        any_b |= b;
        z[bf_pad(i)] = make_float2((float)a, (float)b);
    }
    any_a = __syncthreads_or(any_a);
    any_b = __syncthreads_or(any_b);
    if (any_a && any_b) {
        bf_pass<4, 512, false>(z, tw, tid);
        __syncthreads();
        bf_pass<3, 64, false>(z, tw, tid);
        __syncthreads();
        bf_pass<3, 8, false>(z, tw, tid);
        __syncthreads();
        bf_pass<3, 1, false>(z, tw, tid);
        __syncthreads();
        // Z = A + i B with real a, b:  2 A_k = Z_k + conj(Z_-k),  2 B_k = -i (Z_k - conj(Z_-k));  the factors
        // of 2 drop out of P / |P|.  A thread owns the pair (k, N - k): bins 0 and N / 2 are their own partners.
        for (int k = tid; k <= BF_N / 2; k += BF_TPB) {
            const int p = bf_pad(bf_brev(k)), pm = bf_pad(bf_brev((BF_N - k) & (BF_N - 1)));
            const float2 x = z[p], y = z[pm];
            const float ar = x.x + y.x, ai = x.y - y.y, br = x.y + y.y, bi = y.x - x.x;
            const float pr = br * ar + bi * ai, pi = bi * ar - br * ai;
            const float mag = sqrtf(pr * pr + pi * pi);
            const float2 G = mag > 0.0f ? make_float2(pr / mag, pi / mag) : make_float2(0.0f, 0.0f);
            z[p] = G;
            z[pm] = make_float2(G.x, -G.y);
            if (p == pm) z[p] = make_float2(G.x, 0.0f);     // (P is real there)
        }
        __syncthreads();
        bf_pass<3, 1, true>(z, tw, tid);
        __syncthreads();
        bf_pass<3, 8, true>(z, tw, tid);
        __syncthreads();
        bf_pass<3, 64, true>(z, tw, tid);
        __syncthreads();
        bf_pass<4, 512, true>(z, tw, tid);
        __syncthreads();
    } else {
        for (int i = tid; i < BF_N; i += BF_TPB) z[bf_pad(i)] = make_float2(0.0f, 0.0f);
        __syncthreads();
    }
    // v[d] = r[d mod N] / N for d = i - D
    const float scale = 1.0f / (float)BF_N;
#define BF_V(i) (z[bf_pad(((i) - D) & (BF_N - 1))].x * scale)
    if (cv) for (int i = tid; i < n_lag; i += BF_TPB) cv[i] = BF_V(i);
    float prev_v = INFINITY;
    int prev_l = 0, lag0 = 0;
    for (int k = 0; k < BF_NBEST; ++k) {
        float best_v = -INFINITY;
        int best_l = 0x7fffffff;
        for (int i = tid; i < n_lag; i += BF_TPB) {
            const float v = BF_V(i);
            const bool up = i == 0 || v > BF_V(i - 1), down = i == n_lag - 1 || v >= BF_V(i + 1);
            const int l = i - D;
            if (up && down && (k == 0 || bf_before(prev_v, prev_l, v, l)) && bf_before(v, l, best_v, best_l)) { best_v = v; best_l = l; }
        }
        red_v[tid] = best_v;
        red_l[tid] = best_l;
        __syncthreads();
        for (int o = BF_TPB / 2; o > 0; o >>= 1) {
            if (tid < o && bf_before(red_v[tid + o], red_l[tid + o], red_v[tid], red_l[tid])) {
                red_v[tid] = red_v[tid + o];
                red_l[tid] = red_l[tid + o];
            }
            __syncthreads();
        }
        prev_v = red_v[0];
        prev_l = red_l[0];
        __syncthreads();
        const bool found = prev_l != 0x7fffffff;
        if (k == 0) lag0 = prev_l;
        if (tid == 0) { lag[k] = found ? prev_l : lag0; val[k] = found ? prev_v : -INFINITY; }
        if (!found) {                                   // the later slots are absent too
            if (tid == 0) for (int m = k + 1; m < BF_NBEST; ++m) { lag[m] = lag0; val[m] = -INFINITY; }
            break;
        }
    }
#undef BF_V
}

// One thread per (file, channel).  back[] holds, per step, the four 2-bit back-pointers; delay[] holds the
// step a step takes its lags from (-1: none, the single candidate lag 0) until the backtrack writes the lag.
__global__ void k_bf_track(const long long* __restrict__ wg_off /* sum of T C */, const long long* __restrict__ lane_off /* sum of C */,
                           long long n_files, const int* __restrict__ channels, const int* __restrict__ lag,
                           const float* __restrict__ val, int n_best, float min_peak, double penalty, int cap,
                           unsigned char* __restrict__ back, int* __restrict__ delay) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= lane_off[n_files]) return;
    const long long file = mf_file_of(lane_off, n_files, lane);
    const int C = channels[file], ch = (int)(lane - lane_off[file]);
    const long long T = (wg_off[file + 1] - wg_off[file]) / C;
    lag += wg_off[file] * BF_NBEST;
    val += wg_off[file] * BF_NBEST;
    back += wg_off[file];
    delay += wg_off[file];
    auto at = [&](long long t) { return (t * C + ch) * BF_NBEST; };
    long long first = -1;                               // the first reliable step
    for (long long t = 0; t < T && first < 0; ++t)
        if (val[at(t)] >= min_peak) first = t;
    double S[BF_NBEST];
    int prev_lag[BF_NBEST];
    long long last = -1;                                // the nearest reliable step so far
    for (long long t = 0; t < T; ++t) {
        const bool reliable = val[at(t)] >= min_peak;
        if (reliable) last = t;
        const long long src = reliable ? t : (last >= 0 ? last : first);
        delay[t * C + ch] = (int)src;
        int l[BF_NBEST];
        double v[BF_NBEST];
        for (int k = 0; k < BF_NBEST; ++k) {
            if (src < 0) { l[k] = 0; v[k] = k == 0 ? 0.0 : -INFINITY; continue; }
            const float x = k < n_best ? val[at(src) + k] : -INFINITY;
            l[k] = lag[at(src) + k];
            v[k] = reliable ? (double)x : (x == -INFINITY ? -INFINITY : 0.0);
        }
        unsigned char bp = 0;
        double now[BF_NBEST];
        for (int k = 0; k < BF_NBEST; ++k) {
            if (t == 0) { now[k] = v[k]; continue; }
            double best = 0.0;
            int arg = 0;
            for (int j = 0; j < BF_NBEST; ++j) {
                long long d = (long long)l[k] - (long long)prev_lag[j];
                d = d < 0 ? -d : d;
                d = d < cap ? d : cap;
                const double s = __dsub_rn(S[j], __dmul_rn(penalty, (double)d));
                if (j == 0 || s > best) { best = s; arg = j; }
            }
            now[k] = __dadd_rn(best, v[k]);
            bp |= (unsigned char)(arg << (2 * k));
        }
        back[t * C + ch] = bp;
        for (int k = 0; k < BF_NBEST; ++k) { S[k] = now[k]; prev_lag[k] = l[k]; }
    }
    if (T == 0) return;
    int k = 0;
    for (int j = 1; j < BF_NBEST; ++j)
        if (S[j] > S[k]) k = j;
    for (long long t = T - 1; t >= 0; --t) {
        const int src = delay[t * C + ch];
        delay[t * C + ch] = src < 0 ? 0 : lag[at(src) + k];
        k = (back[t * C + ch] >> (2 * k)) & 3;
    }
}

__device__ inline int16_t bf_round(long long num, long long den) {
    double y = rint((double)num / (double)den);
    y = y < -32768.0 ? -32768.0 : (y > 32767.0 ? 32767.0 : y);
    return (int16_t)(int)y;
}

__global__ __launch_bounds__(BF_SUM_TPB) void k_bf_sum(
        const int16_t* __restrict__ in, const long long* __restrict__ in_off, const long long* __restrict__ out_off,
        const long long* __restrict__ tile_off, const long long* __restrict__ wg_off /* sum of T C */, long long n_files,
        const int* __restrict__ channels, const int* __restrict__ geom_of, const BfGeom* __restrict__ geoms,
        const int* __restrict__ delay, int16_t* __restrict__ out) {
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const int C = channels[file];
    const BfGeom g = geoms[geom_of[file]];
    const long long n = out_off[file + 1] - out_off[file];
    const long long n0 = ((long long)blockIdx.x - tile_off[file]) * BF_SUM_TILE;
    const int cnt = (int)(n - n0 < BF_SUM_TILE ? n - n0 : BF_SUM_TILE);
    in += in_off[file];
    out += out_off[file] + n0;
    if (C == 1) {
        for (int r = threadIdx.x; r < cnt; r += BF_SUM_TPB) out[r] = in[n0 + r];
        return;
    }
    const long long T = (wg_off[file + 1] - wg_off[file]) / C;
    delay += wg_off[file];
    const long long H = g.hop, a0 = g.window / 2, a_last = (T - 1) * H + a0;
    for (int r = threadIdx.x; r < cnt; r += BF_SUM_TPB) {
        const long long s = n0 + r;
        long long t0, t1, j;
        if (s < a0) { t0 = t1 = 0; j = 0; }
        else if (s >= a_last) { t0 = t1 = T - 1; j = 0; }
        else { t0 = (s - a0) / H; t1 = t0 + 1; j = (s - a0) - t0 * H; }
        long long num = 0;
        for (int c = 0; c < C; ++c) {
            const long long i0 = s + delay[t0 * C + c], i1 = s + delay[t1 * C + c];
            const long long x0 = i0 >= 0 && i0 < n ? in[i0 * C + c] : 0, x1 = i1 >= 0 && i1 < n ? in[i1 * C + c] : 0;
            num += (H - j) * x0 + j * x1;
        }
        out[r] = bf_round(num, C * H);
    }
}

}  // namespace spkd
