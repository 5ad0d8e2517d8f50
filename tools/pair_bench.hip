// Where does a production pass lose time against the bare elimination?  BIC pair
// distances of one row record (LDS) with a window of partner quad records (global):
//   mode 0  the bare symmetric elimination (formation + tri_det_nopivot + log), as in
//           blocked_bench.hip
//   mode 1  the library's quad_pair_det<false> + log + finish_distance + a store, in every pass
//           (k_matrix's pass until the dense finish)
//   mode 2  the bare elimination from packed records;  mode 3  the same, register-pipelined
//   mode 4  k_matrix's body: quad_pair_det<false> per pass, the determinant parked in the output
//           cell; then a barrier and log + finish_distance by one thread per partner
// each with the partner records L2-resident (n_rec = 387) and streaming from HBM
// (n_rec = 40 000, every block a different window of 387 partners).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I../speaker-diarization_amd/csrc -o pair_bench pair_bench.hip
// The row split follows spkd_quad.hpp; the even split for comparison: add -DSPKD_QUAD_BASES=0,13,26
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "spkd_cluster.hpp"
#include "spkd_tri.hpp"
#include "packed_columns.hpp"
using namespace spkd;

constexpr int WINDOW = 387;

template <int MODE>
__global__ __launch_bounds__(512) void k_pairs(const double* __restrict__ qr, int n_rec, const double* __restrict__ ld,
                                               double* __restrict__ out, int* err, const double* __restrict__ pk = nullptr) {
    __shared__ double ldsA[QREC];
    const int wave = threadIdx.x >> 6;
    const QuadLane L = quad_lane();
    const int a = (int)(((long long)blockIdx.x * 97) % n_rec);
    const double* A = qr + (size_t)a * QREC;
    for (int e = threadIdx.x; e < QREC; e += blockDim.x) ldsA[e] = A[e];
    __syncthreads();
    const double nA = ldsA[QREC_COUNT_AT];
    const double ldA = ld[a];
    double acc = 0.0;
    if (MODE == 3) {
        // bare elimination, packed records, software-pipelined in registers: column K of the
        // NEXT record is loaded into the registers step K of this elimination has just freed
        int ta = L.t; asm volatile("" : "+v"(ta));
        const int t12 = quad_load_lane(ta);
        auto rec_of = [&](int base) -> const double* {
            int w = base + L.m;
            w = w < WINDOW ? w : WINDOW - 1;
            return pk + (size_t)((a + 1 + w) % n_rec) * REC;
        };
        QuadRows q, qn; double sv[QS], svn[QS];
        PackedColumns pc;
        int base = 4 * wave;
        const double* P = rec_of(base);
        pc.dst = &q; pc.sums = sv; pc.set_record(P, t12);
        pc.all();
        double cnt = P[REC - 1];
        for (; base < WINDOW; base += 32) {
            const double* Pn = rec_of(base + 32 < WINDOW ? base + 32 : base);
            const double cnt_n = Pn[REC - 1];
            pc.dst = &qn; pc.sums = svn; pc.set_record(Pn, t12);
            const double n = nA + cnt;
            const double f = 1.0 / (n - 1.0);
            double c1[QS];
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) {
#pragma unroll
                for (int j = 0; j < tri_cols(s2); ++j) q.r[s2][j] = f * (ldsA[(s2 * DA + j) * 16 + ta] + q.r[s2][j]);
                sv[s2] = ldsA[(s2 * DA + D) * 16 + ta] + sv[s2];
                c1[s2] = -((f / n) * sv[s2]);
                __builtin_amdgcn_sched_barrier(0);
            }
            TriRank1<0>::run(q, c1, sv);
            double det; tri_det_nopivot(q, det, pc);
            acc += log(det);
            q = qn;
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) sv[s2] = svn[s2];
            cnt = cnt_n;
        }
        if (L.t == 0) out[(size_t)blockIdx.x * WINDOW + wave * 4 + L.m] = acc;
        return;
    }
    if (MODE == 4) {
        double* row = out + (size_t)blockIdx.x * WINDOW;
        for (int base = 4 * wave; base < WINDOW; base += 32) {
            int w = base + L.m;
            const bool valid = w < WINDOW;
            w = valid ? w : WINDOW - 1;
            const int rc = (a + 1 + w) % n_rec;
            const double det = quad_pair_det<false>(SPKD_BIC, ldsA, nA, A, qr + (size_t)rc * QREC, pk + (size_t)rc * REC, false, L, err);
            if (valid && L.t == 0) row[w] = det;
        }
        __syncthreads();
        for (int w = threadIdx.x; w < WINDOW; w += blockDim.x) {
            const int rc = (a + 1 + w) % n_rec;
            row[w] = finish_distance(SPKD_BIC, 1.3, nA, ldA, pk[(size_t)rc * REC + REC - 1], ld[rc], log(row[w]));
        }
        return;
    }
    for (int base = 4 * wave; base < WINDOW; base += 32) {
        int w = base + L.m;
        const bool valid = w < WINDOW;
        w = valid ? w : WINDOW - 1;
        const int rc = (a + 1 + w) % n_rec;
        const double* C = qr + (size_t)rc * QREC;
        if (MODE == 2) {
            // bare elimination, partner records in the packed ABI layout (6 560 B)
            const double* P = pk + (size_t)rc * REC;
            QuadRows q; double sv[QS];
            int ta = L.t; asm volatile("" : "+v"(ta));
            const double n = nA + P[REC - 1];
            const double f = 1.0 / (n - 1.0);
            const int t12 = quad_load_lane(ta);
            const double* rt[2];
            long long o1 = 512; asm volatile("" : "+v"(o1));
            rt[0] = P + t12; rt[1] = rt[0] + o1;
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) {
#pragma unroll
                for (int j = 0; j < tri_cols(s2); ++j) { const int e = quad_pk_at(s2, j); q.r[s2][j] = rt[e / 512][e % 512]; }
                const int c = quad_row(s2, t12);
                sv[s2] = P[pk_off(c) + D - c];
            }
            __builtin_amdgcn_sched_barrier(0);
            double c1[QS];
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) {
#pragma unroll
                for (int j = 0; j < tri_cols(s2); ++j) q.r[s2][j] = f * (ldsA[(s2 * DA + j) * 16 + ta] + q.r[s2][j]);
                sv[s2] = ldsA[(s2 * DA + D) * 16 + ta] + sv[s2];
                c1[s2] = -((f / n) * sv[s2]);
                __builtin_amdgcn_sched_barrier(0);
            }
            TriRank1<0>::run(q, c1, sv);
            double det; tri_det_nopivot(q, det);
            acc += log(det);
        } else if (MODE == 0) {
            QuadRows q; double sv[QS];
            int ta = L.t; asm volatile("" : "+v"(ta));
            const double n = nA + C[QREC_COUNT_AT];
            const double f = 1.0 / (n - 1.0);
            const double* Ct = C + L.t;
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) {
#pragma unroll
                for (int j = 0; j < tri_cols(s2); ++j) q.r[s2][j] = Ct[(s2 * DA + j) * 16];
                sv[s2] = Ct[(s2 * DA + D) * 16];
            }
            __builtin_amdgcn_sched_barrier(0);
            double c1[QS];
#pragma unroll
            for (int s2 = 0; s2 < QS; ++s2) {
#pragma unroll
                for (int j = 0; j < tri_cols(s2); ++j) q.r[s2][j] = f * (ldsA[(s2 * DA + j) * 16 + ta] + q.r[s2][j]);
                sv[s2] = ldsA[(s2 * DA + D) * 16 + ta] + sv[s2];
                c1[s2] = -((f / n) * sv[s2]);
                __builtin_amdgcn_sched_barrier(0);
            }
            TriRank1<0>::run(q, c1, sv);
            double det; tri_det_nopivot(q, det);
            acc += log(det);
        } else {
            const double ldx = log(quad_pair_det<false>(SPKD_BIC, ldsA, nA, A, C, pk + (size_t)rc * REC, false, L, err));
            const double d = finish_distance(SPKD_BIC, 1.3, nA, ldA, qr_count(C), ld[rc], ldx);
            if (valid && L.t == 0) out[(size_t)blockIdx.x * WINDOW + w] = d;
            acc += d;
        }
    }
    if (MODE != 1 && L.t == 0) out[(size_t)blockIdx.x * WINDOW + wave * 4 + L.m] = acc;
}

int main(int argc, char** argv) {
    const int blocks = argc > 1 ? atoi(argv[1]) : 4096;
    for (int n_rec : {387, 40000}) {
        std::vector<double> h((size_t)n_rec * QREC, 0.0), hld(n_rec, 0.0);
        srand(2);
        std::vector<double> M(DA * DA);
        for (int r = 0; r < n_rec; ++r) {
            // a handful of generated records, repeated with a small perturbation of the counts
            const int nf = 300 + (r % 7) * 100;
            if (r < 64) {
                std::fill(M.begin(), M.end(), 0.0);
                for (int f = 0; f < nf; ++f) {
                    double x[DA];
                    for (int i = 0; i < D; ++i) x[i] = (rand() / (double)RAND_MAX) - 0.5 + 0.01 * r;
                    x[D] = 1.0;
                    for (int i = 0; i < DA; ++i) for (int j = 0; j < DA; ++j) M[j * DA + i] += x[i] * x[j];
                }
                double* o = &h[(size_t)r * QREC];
                for (int i = 0; i < D; ++i) for (int j = 0; j < DA; ++j) o[qr_index(i, j)] = M[j * DA + i];
                o[QREC_COUNT_AT] = nf;
            } else {
                std::copy(&h[(size_t)(r % 64) * QREC], &h[(size_t)(r % 64 + 1) * QREC], &h[(size_t)r * QREC]);
            }
            hld[r] = -30.0 - 0.01 * (r % 64);
        }
        // packed copies of the same records
        std::vector<double> hp((size_t)n_rec * REC, 0.0);
        for (int r = 0; r < n_rec; ++r) {
            const double* o = &h[(size_t)r * QREC];
            double* pr = &hp[(size_t)r * REC];
            for (int j = 0; j < DA; ++j) for (int i = j; i < DA; ++i) {
                double v;
                if (i < D) v = o[qr_index(i, j)];
                else if (j < D) v = o[qr_index(j, D)];     // sums
                else v = o[QREC_COUNT_AT];
                pr[pk_off(j) + (i - j)] = v;
            }
        }
        double *dE, *dO, *dL, *dP; int* dErr;
        hipMalloc(&dP, hp.size() * 8); hipMemcpy(dP, hp.data(), hp.size() * 8, hipMemcpyHostToDevice);
        hipMalloc(&dE, h.size() * 8); hipMalloc(&dO, (size_t)blocks * WINDOW * 8 + 4096); hipMalloc(&dL, n_rec * 8); hipMalloc(&dErr, 4);
        hipMemcpy(dE, h.data(), h.size() * 8, hipMemcpyHostToDevice);
        hipMemcpy(dL, hld.data(), n_rec * 8, hipMemcpyHostToDevice);
        hipMemset(dErr, 0, 4);
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        for (int mode = 0; mode < 5; ++mode)
            for (int it = 0; it < 3; ++it) {
                hipEventRecord(e0);
                if (mode == 0) hipLaunchKernelGGL(k_pairs<0>, dim3(blocks), dim3(512), 0, 0, dE, n_rec, dL, dO, dErr, (const double*)nullptr);
                else if (mode == 1) hipLaunchKernelGGL(k_pairs<1>, dim3(blocks), dim3(512), 0, 0, dE, n_rec, dL, dO, dErr, (const double*)dP);
                else if (mode == 2) hipLaunchKernelGGL(k_pairs<2>, dim3(blocks), dim3(512), 0, 0, dE, n_rec, dL, dO, dErr, (const double*)dP);
                else if (mode == 3) hipLaunchKernelGGL(k_pairs<3>, dim3(blocks), dim3(512), 0, 0, dE, n_rec, dL, dO, dErr, (const double*)dP);
                else hipLaunchKernelGGL(k_pairs<4>, dim3(blocks), dim3(512), 0, 0, dE, n_rec, dL, dO, dErr, (const double*)dP);
                hipEventRecord(e1); hipEventSynchronize(e1);
                float ms; hipEventElapsedTime(&ms, e0, e1);
                if (it == 2) printf("n_rec %6d  %-37s %.3f ms  %.1f M pairs/s\n", n_rec,
                                    mode == 0 ? "bare elimination" : (mode == 1 ? "quad_pair_det + log + finish_distance" : (mode == 2 ? "bare elimination, packed records" : (mode == 3 ? "bare, packed, register-pipelined" : "quad_pair_det parked + dense finish"))), ms,
                                    (double)blocks * WINDOW / ms / 1e3);
            }
        hipFree(dP); hipFree(dE); hipFree(dO); hipFree(dL); hipFree(dErr);
    }
    return 0;
}
