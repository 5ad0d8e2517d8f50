// Speech / non-speech frame scoring for the generate_exp.py stand-in (exp_generator.py):
// per frame, the natural-log density of every HMM state's diagonal-covariance Gaussian mixture,
//
//   score[t][s] = logsumexp_{k in s} ( ln w_sk + c_k - 1/2 sum_d (x_td - mu_kd)^2 iv_kd ),
//   c_k = -1/2 (D ln 2pi + sum_d ln v_kd)          (c_k, iv = 1/v, ln w from the host, fp64 -> fp32)
//
// PARITY UNPINNED (AaltoASR's phone_probs is not available): the convention is the one listed in
// include/spkd.h and restated in the test suite's numpy file.
//
//   k_gmm_loglik : one frame per lane, GM_TPB frames per workgroup.  The workgroup's frames are
//                  staged through LDS with coalesced loads (39 floats per frame, contiguous), each
//                  lane keeps its frame in registers; the model (a few KB) is indexed by the
//                  state / kernel loop counters only, so every lane reads the same address and the
//                  loads go down the scalar path.  A state's log-sum-exp takes its maximum first
//                  (two passes over its kernels: the quadratic forms are recomputed instead of
//                  kept, K is not known at compile time).  The [GM_TPB][S] result goes back
//                  through the same LDS tile so that the stores are coalesced too.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spkd {

constexpr int GM_DIM = 39;
constexpr int GM_TPB = 256;          // frames per workgroup (one per lane)
constexpr int GM_MAX_K = 256;        // kernels per model
constexpr int GM_MAX_S = 16;         // states per model

__device__ inline float gm_term(const float (&x)[GM_DIM], const float* __restrict__ mean,
                                const float* __restrict__ iv, const float* __restrict__ cnorm, int k, float lw) {
    const float* mu = mean + k * GM_DIM;
    const float* v = iv + k * GM_DIM;
    float q = 0.0f;
#pragma unroll
    for (int d = 0; d < GM_DIM; ++d) {
        const float e = x[d] - mu[d];
        q = fmaf(e * e, v[d], q);
    }
    return lw + (cnorm[k] - 0.5f * q);
}

__global__ __launch_bounds__(GM_TPB) void k_gmm_loglik(
        const float* __restrict__ feat /* [T][39] */, long long n_frames,
        const float* __restrict__ mean /* [K][39] */, const float* __restrict__ iv /* [K][39] */,
        const float* __restrict__ cnorm /* [K] */, const int* __restrict__ state_off /* [S+1] */,
        const int* __restrict__ kernel /* [nnz] */, const float* __restrict__ log_weight /* [nnz] */, int n_states,
        float* __restrict__ score /* [T][S] */) {
    __shared__ float tile[GM_TPB * GM_DIM];
    const int tid = threadIdx.x;
    const long long f0 = (long long)blockIdx.x * GM_TPB;
    const long long left = n_frames - f0;
    const int nf = left < GM_TPB ? (int)left : GM_TPB;          // frames of this workgroup
    const float* src = feat + f0 * GM_DIM;
    for (int e = tid; e < nf * GM_DIM; e += GM_TPB) tile[e] = src[e];
    __syncthreads();
    float x[GM_DIM];
#pragma unroll
    for (int d = 0; d < GM_DIM; ++d) x[d] = tid < nf ? tile[tid * GM_DIM + d] : 0.0f;
    __syncthreads();                                             // the tile is reused for the scores
    for (int s = 0; s < n_states; ++s) {
        const int b = state_off[s], e = state_off[s + 1];
        float m = -INFINITY;
        bool any = false, nan = false;
        for (int j = b; j < e; ++j) {
            const float lw = log_weight[j];
            if (lw == -INFINITY) continue;                       // a weight of 0 contributes nothing
            const float t = gm_term(x, mean, iv, cnorm, kernel[j], lw);
            any = true;
            nan |= t != t;
            m = fmaxf(m, t);
        }
        float r;
        if (!any || (m == -INFINITY && !nan)) {
            r = -INFINITY;                                       // no term, or every term -inf
        } else if (nan) {
            r = __builtin_nanf("");
        } else {
            float sum = 0.0f;
            for (int j = b; j < e; ++j) {
                const float lw = log_weight[j];
                if (lw == -INFINITY) continue;
                sum += expf(gm_term(x, mean, iv, cnorm, kernel[j], lw) - m);
            }
            r = m + logf(sum);
        }
        tile[tid * n_states + s] = r;
    }
    __syncthreads();
    float* dst = score + f0 * n_states;
    for (int e = tid; e < nf * n_states; e += GM_TPB) dst[e] = tile[e];
}

}  // namespace spkd
