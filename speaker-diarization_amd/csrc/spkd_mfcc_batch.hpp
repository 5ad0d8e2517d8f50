// The front-end's kernels (spkd_mfcc_batch; spkd_mfcc is the batch of one file): the samples of
// n_files files concatenated, file f at [sample_off[f], sample_off[f+1]), its T_f = n_f / hop frames
// at [frame_off[f], frame_off[f+1]) of the static rows and of the features.  A workgroup's tile of
// frames lies in one file: the host counts the tiles of every file into a prefix table, a workgroup
// finds its file there by a binary search on its block index (the same in every lane) and works on
// the file's own samples and rows, so every border rule is the file's and nothing of a neighbour
// is read.
//
//   k_mfcc_tables : once per call, the values every tile needs -- the 512 twiddles (float2,
//                   padded: mf_tw_slot) and the WIN Hamming weights (fp64) -- by the device's own
//                   cos / sin, so a tile fetches them instead of evaluating 1 024 + 3 200 fp64
//                   functions.
//   k_mfcc_static : templated on the window width (400: fconfig.cfg; 256: the VAD model's .cfg,
//                   zero-padded to the same 512-point transform).  Workgroup per MF_FR = 8 frames
//                   of one file, 5 waves.  Pre-emphasis + Hamming window into LDS as y[n][frame],
//                   then a direct 512-point DFT: thread k of waves 0..3 is bin k, per sample one
//                   8-byte twiddle read and the 8 frames' values from two 16-byte reads for 16
//                   FMAs; wave 4 does bin 256, a lane per frame (on wave 0 it was a second pass of
//                   a whole wave).  Each (frame, bin) is the serial fmaf chain over n = 0 .. WIN-1.
//                   Magnitude, mel filterbank, log, DCT, log power -> static [T][13].
//                   Measured on an MI355X: 3.0 ms per audio-hour (2.2 for 256-sample windows).
//   k_mfcc_post   : workgroup per MP_FR = 128 frames of one file.  The static rows it needs (+-75
//                   for the mean, +-4 for the two delta stages) staged in LDS once; cms, deltas,
//                   normalization and the 39x39 transform from there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spkd_mfcc.hpp"

namespace spkd {

constexpr int MF_STATIC_TPB = MF_TPB + 64;     // the bins 0 .. 255, and a wave for bin 256
static_assert(MF_FR == 8, "k_mfcc_static reads a sample's frames as two float4");
static_assert(MF_BINS == MF_TPB + 1, "one thread per bin below the last");

// the file of tile b: tile_off[f] <= b < tile_off[f + 1] (files without a tile repeat an offset)
__device__ inline long long mf_file_of(const long long* __restrict__ tile_off, long long n_files, long long b) {
    long long lo = 0, hi = n_files;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) / 2;
        if (tile_off[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

template <int WIN>
__global__ __launch_bounds__(MF_NFFT) void k_mfcc_tables(float2* __restrict__ tw /* [MF_TW_LEN] */,
                                                         double* __restrict__ ham /* [WIN] */) {
    const int n = threadIdx.x;
    tw[mf_tw_slot(n)] = mf_twiddle(n);
    if (n < WIN) ham[n] = mf_hamming<WIN>(n);
}

template <int WIN>
__global__ __launch_bounds__(MF_STATIC_TPB) void k_mfcc_static(
        const int16_t* __restrict__ pcm, const long long* __restrict__ sample_off, const long long* __restrict__ frame_off,
        const long long* __restrict__ tile_off /* [n_files + 1] each */, long long n_files, int hop, float pre_emph,
        const float2* __restrict__ g_tw, const double* __restrict__ g_ham, const float* __restrict__ melfb /* [MF_MEL][MF_BINS] */,
        const float* __restrict__ dct /* [MF_CEP][MF_MEL] */, float* __restrict__ stat /* [sum T][13] */) {
    static_assert(WIN <= MF_NFFT, "the window is zero-padded to the transform length");
    __shared__ float4 y[WIN][MF_FR / 4];
    __shared__ float2 tw[MF_TW_LEN];
    __shared__ float mag[MF_FR][MF_BINS + 3];
    __shared__ float lmel[MF_FR][MF_MEL + 3];
    __shared__ float pw[MF_FR][MF_TPB / 64];
    const int tid = threadIdx.x;
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const long long n_samples = sample_off[file + 1] - sample_off[file];
    const long long n_frames = frame_off[file + 1] - frame_off[file];
    const long long t0 = ((long long)blockIdx.x - tile_off[file]) * MF_FR;      // in the file
    pcm += sample_off[file];
    stat += frame_off[file] * MF_STATIC;
    for (int n = tid; n < MF_TW_LEN; n += MF_STATIC_TPB) tw[n] = g_tw[n];
    float* yf = (float*)y;                                                     // [WIN][MF_FR]
    // neighbouring lanes take neighbouring samples of one frame (the reads coalesce); the store transposes
    for (int e = tid; e < MF_FR * WIN; e += MF_STATIC_TPB) {
        const int f = e / WIN, n = e - f * WIN;
        const long long t = t0 + f;
        yf[n * MF_FR + f] = t < n_frames ? mf_sample(pcm, n_samples, t * hop - WIN / 2 + n, pre_emph, g_ham[n]) : 0.0f;
    }
    __syncthreads();
    if (tid < MF_TPB) {
        const int k = tid;
        float re[MF_FR], im[MF_FR];
#pragma unroll
        for (int f = 0; f < MF_FR; ++f) { re[f] = 0.0f; im[f] = 0.0f; }
        int ph = 0;                                   // (k * n) mod 512
#pragma unroll 4
        for (int n = 0; n < WIN; ++n) {
            const float2 cs = tw[mf_tw_slot(ph)];
            ph = (ph + k) & (MF_NFFT - 1);
            const float4 a = y[n][0], b = y[n][1];
            const float v[MF_FR] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int f = 0; f < MF_FR; ++f) mf_dft_step(v[f], cs, re[f], im[f]);
        }
#pragma unroll
        for (int f = 0; f < MF_FR; ++f) mag[f][k] = mf_magnitude(re[f], im[f]);
    } else if (tid < MF_TPB + MF_FR) {
        const int f = tid - MF_TPB;
        float re = 0.0f, im = 0.0f;
        int ph = 0;
        for (int n = 0; n < WIN; ++n) {
            const float2 cs = tw[mf_tw_slot(ph)];
            ph = (ph + MF_TPB) & (MF_NFFT - 1);
            mf_dft_step(yf[n * MF_FR + f], cs, re, im);
        }
        mag[f][MF_TPB] = mf_magnitude(re, im);
    }
    __syncthreads();
    // log power: sum of squared magnitudes (thread k < 256: bin k, thread 0 bin 256 after it; wave
    // partials, then 4 values per frame)
    if (tid < MF_TPB)
        for (int f = 0; f < MF_FR; ++f) {
            float p = 0.0f;
            for (int k = tid; k < MF_BINS; k += MF_TPB) p = fmaf(mag[f][k], mag[f][k], p);
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) p += __shfl_xor(p, s);
            if ((tid & 63) == 0) pw[f][tid >> 6] = p;
        }
    // mel filterbank + log: thread (f, m)
    if (tid < MF_FR * MF_MEL) {
        const int f = tid / MF_MEL, m = tid - f * MF_MEL;
        lmel[f][m] = mf_log_mel(melfb + m * MF_BINS, mag[f]);
    }
    __syncthreads();
    // DCT (cepstra 1..12) and the power column: thread (f, c)
    if (tid < MF_FR * MF_STATIC) {
        const int f = tid / MF_STATIC, c = tid - f * MF_STATIC;
        const long long t = t0 + f;
        if (t < n_frames) {
            float v;
            if (c < MF_CEP) {
                v = mf_cepstrum(dct + c * MF_MEL, lmel[f]);
            } else {
                float p = 0.0f;
                for (int w = 0; w < MF_TPB / 64; ++w) p += pw[f][w];
                v = logf(fmaxf(p, MF_FLOOR));
            }
            stat[t * MF_STATIC + c] = v;
        }
    }
}

__global__ __launch_bounds__(MF_TPB) void k_mfcc_post(
        const float* __restrict__ stat, const long long* __restrict__ frame_off, const long long* __restrict__ tile_off,
        long long n_files, int cms_left, int cms_right, int w1, float norm1, int w2, float norm2,
        const float* __restrict__ mean, const float* __restrict__ scale, const float* __restrict__ transform,
        float* __restrict__ out /* [sum T][39] */) {
    extern __shared__ float mp_lds[];
    const int span = MP_SPAN;                              // frames whose cms / deltas are formed here
    const int raw_n = span + cms_left + cms_right;         // static rows staged
    float* raw = mp_lds;                                   // [raw_n][13]
    float* cms = raw + raw_n * MF_STATIC;                  // [span][13]
    float* d1 = cms + span * MF_STATIC;                    // [span][13]
    float* z = d1 + span * MF_STATIC;                      // [MP_FR][39]
    float* tr = z + MP_FR * MF_DIM;                        // [39][39]
    const int tid = threadIdx.x;
    // from here on every frame number is the file's own
    const long long file = mf_file_of(tile_off, n_files, blockIdx.x);
    const long long n_frames = frame_off[file + 1] - frame_off[file];
    stat += frame_off[file] * MF_STATIC;
    out += frame_off[file] * MF_DIM;
    const long long t0 = ((long long)blockIdx.x - tile_off[file]) * MP_FR;
    const long long first = t0 - MP_HALO;                  // frame of span index 0
    const long long raw0 = first - cms_left;               // frame of raw row 0
    for (int e = tid; e < raw_n * MF_STATIC; e += MF_TPB) {
        const int r = e / MF_STATIC, c = e - r * MF_STATIC;
        const long long g = raw0 + r;
        raw[e] = (g >= 0 && g < n_frames) ? stat[g * MF_STATIC + c] : 0.0f;
    }
    for (int e = tid; e < MF_DIM * MF_DIM; e += MF_TPB) tr[e] = transform[e];
    __syncthreads();
    auto clampg = [&](long long g) { return g < 0 ? 0 : (g >= n_frames ? n_frames - 1 : g); };
    // cms of span frame i = static - mean over the existing frames of [g - left, g + right]
    for (int e = tid; e < span * MF_STATIC; e += MF_TPB) {
        const int i = e / MF_STATIC, c = e - i * MF_STATIC;
        const long long g = clampg(first + i);             // frames beyond the file repeat the border frame
        long long lo = g - cms_left, hi = g + cms_right + 1;
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_frames ? n_frames : hi;
        double s = 0.0;
        for (long long q = lo; q < hi; ++q) s += (double)raw[(q - raw0) * MF_STATIC + c];
        cms[e] = (float)((double)raw[(g - raw0) * MF_STATIC + c] - s / (double)(hi - lo));
    }
    __syncthreads();
    // d1 over the span (index clamps happen on the FILE's frame numbers, like the restatement)
    for (int e = tid; e < span * MF_STATIC; e += MF_TPB) {
        const int i = e / MF_STATIC, c = e - i * MF_STATIC;
        const long long g = clampg(first + i);
        float v = 0.0f;
        for (int k = 1; k <= w1; ++k) {
            const long long a = clampg(g + k) - first, b = clampg(g - k) - first;
            const bool ok = a >= 0 && a < span && b >= 0 && b < span;
            v += ok ? (float)k * (cms[a * MF_STATIC + c] - cms[b * MF_STATIC + c]) : 0.0f;
        }
        d1[e] = v / norm1;
    }
    __syncthreads();
    for (int e = tid; e < MP_FR * MF_STATIC; e += MF_TPB) {
        const int f = e / MF_STATIC, c = e - f * MF_STATIC;
        const long long g = t0 + f;
        if (g >= n_frames) continue;
        const int i = f + MP_HALO;
        float v = 0.0f;
        for (int k = 1; k <= w2; ++k) {
            const long long a = clampg(g + k) - first, b = clampg(g - k) - first;
            v += (float)k * (d1[a * MF_STATIC + c] - d1[b * MF_STATIC + c]);
        }
        const float d2 = v / norm2;
        z[f * MF_DIM + c] = (cms[i * MF_STATIC + c] - mean[c]) * scale[c];
        z[f * MF_DIM + MF_STATIC + c] = (d1[i * MF_STATIC + c] - mean[MF_STATIC + c]) * scale[MF_STATIC + c];
        z[f * MF_DIM + 2 * MF_STATIC + c] = (d2 - mean[2 * MF_STATIC + c]) * scale[2 * MF_STATIC + c];
    }
    __syncthreads();
    for (int e = tid; e < MP_FR * MF_DIM; e += MF_TPB) {
        const int f = e / MF_DIM, r = e - f * MF_DIM;
        const long long g = t0 + f;
        if (g >= n_frames) continue;
        float v = 0.0f;
        for (int c = 0; c < MF_DIM; ++c) v = fmaf(tr[r * MF_DIM + c], z[f * MF_DIM + c], v);
        out[g * MF_DIM + r] = v;
    }
}

}  // namespace spkd
