// Register-pipelined record loads for the symmetric elimination of spkd_tri.hpp.  The library
// does not use them (inside k_gw the compiler could not hold them: DESIGN.md par. 3); kept for
// tools/pair_bench.hip mode 3, which measures them against the bare passes.
#pragma once
#include "spkd_tri.hpp"

namespace spkd {

// A hook for tri_det / tri_det_nopivot: the lower-triangle columns of a PACKED record (SPKD_REC doubles:
// column j holds rows j .. 39 contiguously from pk_off(j), so the quad load of (slot s,
// column j) is 16 consecutive doubles at quad_pk_at(s, j) + t; lanes without a row read
// inside the record, into registers nobody reads: spkd_quad.hpp) -> `dst`, column K after step K; the sums column (three more
// doubles per lane) comes with column SUMS_AT, late enough to cost no register while the
// matrix is still large and early enough to have landed when the elimination ends.
// rt0 = record + t (t = quad_load_lane(lane in the DPP row)), rt1 = rt0 + 512: the immediate offset
// of a global load spans 4 KB, so two bases reach the whole record.
struct PackedColumns {
    static constexpr int SUMS_AT = quad_base(2);
    const SPKD_GLOBAL double* rt0;
    const SPKD_GLOBAL double* rt1;
    QuadRows* dst;
    double* sums;         // [QS]

    __device__ __forceinline__ void set_record(const double* rec, int t12) {
        long long o1 = 512;                 // opaque, so that the bases stay separate registers
        asm volatile("" : "+v"(o1));
        rt0 = (const SPKD_GLOBAL double*)rec + t12;
        rt1 = rt0 + o1;
    }
    template <int J>
    __device__ __forceinline__ void column() {
#pragma unroll
        for (int s = quad_slot(J); s < QS; ++s) {
            const int e = quad_pk_at(s, J);             // + t (in the base)
            dst->r[s][J] = e < 512 ? rt0[e] : rt1[e - 512];
        }
    }
    // (39, c) for this lane's row c = quad_row(s, t) of slot s: record[pk_off(c) + 39 - c]
    __device__ __forceinline__ void sums_column() {
        int t = lane_id() & 15;
        t = quad_load_lane(t);
#pragma unroll
        for (int s = 0; s < QS; ++s) {
            const int c = quad_row(s, t);
            sums[s] = rt0[pk_off(c) + D - c - t];
        }
    }
    template <int K>
    __device__ __forceinline__ void after_step() {
        column<K>();
        if constexpr (K == SUMS_AT) sums_column();
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void redo() { all(); }
    // the whole record at once (the first pass of a loop: nothing to hide the loads under)
    template <int J = 0>
    __device__ __forceinline__ void all() {
        if constexpr (J < D) {
            column<J>();
            all<J + 1>();
        } else {
            sums_column();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

}  // namespace spkd
