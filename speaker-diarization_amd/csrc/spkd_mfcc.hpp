// feacat-shaped MFCC front-end: 16-bit PCM -> float32 [T][39]
// features per the reference's fconfig.cfg (audiofile -> fft magnitude -> mel / power ->
// dct 12 -> cms +-75 -> delta, delta-delta -> normalization -> 39x39 transform).
// PARITY UNPINNED (feacat is not available): the module semantics the configuration file
// does not spell out are the choices listed in oracle/mfcc_numpy.py, which this restates.
//
// This file: the sizes and the per-frame arithmetic, each expression stated once.  The
// kernels that run it over the files of a batch are in spkd_mfcc_batch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spkd {

constexpr int MF_WIN = 400;          // samples per window (fconfig.cfg)
constexpr int MF_WIN_VAD = 256;      // samples per window (the VAD model's .cfg)
constexpr int MF_NFFT = 512;
constexpr int MF_BINS = MF_NFFT / 2 + 1;
constexpr int MF_MEL = 21;
constexpr int MF_CEP = 12;
constexpr int MF_STATIC = MF_CEP + 1;
constexpr int MF_DIM = 3 * MF_STATIC;          // 39
constexpr int MF_FR = 8;             // frames per workgroup (static stage)
constexpr int MF_TPB = 256;
constexpr float MF_FLOOR = 1e-10f;
constexpr int MP_FR = 128;           // frames per workgroup (post stage)
constexpr int MP_HALO = 4;           // two delta stages of width 2
constexpr int MP_SPAN = MP_FR + 2 * MP_HALO;   // frames whose cms / first deltas a post tile forms
constexpr int MP_LDS_MAX = 60 * 1024;          // bytes of LDS a post tile may take (SPKD_MFCC_POST_LDS)

// floats of LDS of a post tile whose mean window is left + right = cms frames wide: the staged
// static rows, cms and d1 over the span, the normalized rows, the transform (k_mfcc_post carves
// them in this order)
__host__ __device__ constexpr int mp_lds_floats(int cms) {
    return (MP_SPAN + cms) * MF_STATIC + 2 * MP_SPAN * MF_STATIC + MP_FR * MF_DIM + MF_DIM * MF_DIM;
}
// the widest mean window, left + right, that fits (SPKD_MFCC_CMS_MAX)
constexpr int MP_CMS_MAX = (MP_LDS_MAX / (int)sizeof(float) - mp_lds_floats(0)) / MF_STATIC;
static_assert(mp_lds_floats(MP_CMS_MAX) * sizeof(float) <= MP_LDS_MAX &&
              mp_lds_floats(MP_CMS_MAX + 1) * sizeof(float) > MP_LDS_MAX, "MP_CMS_MAX is the last width that fits");

// The twiddle table is padded by one entry per 32: a lane of bin k reads entry k n mod 512, and
// for n a multiple of 16 a plain table has the 32 lanes of a group on one LDS bank.
constexpr int MF_TW_LEN = MF_NFFT + MF_NFFT / 32;
__host__ __device__ constexpr int mf_tw_slot(int p) { return p + (p >> 5); }

constexpr double MF_TWO_PI = 6.283185307179586476925286766559;

// (cos, sin) of 2 pi n / 512, formed in fp64
__device__ inline float2 mf_twiddle(int n) {
    const double a = MF_TWO_PI * (double)n / (double)MF_NFFT;
    return make_float2((float)cos(a), (float)sin(a));
}

// Hamming weight n of a WIN-sample window, fp64
template <int WIN>
__device__ inline double mf_hamming(int n) {
    return 0.54 - 0.46 * cos(MF_TWO_PI * (double)n / (double)(WIN - 1));
}

// pre-emphasised, windowed sample i of a file of n_samples (indices clamp to the file)
__device__ inline float mf_sample(const int16_t* __restrict__ pcm, long long n_samples, long long i, float pre_emph,
                                  double w) {
    const long long ic = i < 0 ? 0 : (i >= n_samples ? n_samples - 1 : i);
    const long long ip = i - 1 < 0 ? 0 : (i - 1 >= n_samples ? n_samples - 1 : i - 1);
    return (float)(((double)pcm[ic] - (double)pre_emph * (double)pcm[ip]) * w);
}

// one term of a bin's serial chain over n = 0 .. WIN-1
__device__ inline void mf_dft_step(float v, float2 cs, float& re, float& im) {
    re = fmaf(v, cs.x, re);
    im = fmaf(-v, cs.y, im);
}

__device__ inline float mf_magnitude(float re, float im) { return sqrtf(re * re + im * im); }

// log mel energy m of a frame's magnitudes
__device__ inline float mf_log_mel(const float* __restrict__ w /* melfb row [MF_BINS] */, const float* mag) {
    float acc = 0.0f;
    for (int k = 0; k < MF_BINS; ++k) acc = fmaf(w[k], mag[k], acc);
    return logf(fmaxf(acc, MF_FLOOR));
}

// cepstrum c (1-based row c of the DCT) of a frame's log mel energies
__device__ inline float mf_cepstrum(const float* __restrict__ d /* dct row [MF_MEL] */, const float* lmel) {
    float v = 0.0f;
    for (int m = 0; m < MF_MEL; ++m) v = fmaf(d[m], lmel[m], v);
    return v;
}

}  // namespace spkd
