// Quad layout: FOUR 39x39 matrices per wave64, one per 16-lane DPP row.
//
// Inside a DPP row every lane holds up to three rows of its matrix, one per slot.  The
// rows are split 7 / 16 / 16 over the slots:
//     slot 0: rows  0 ..  6 in lanes 0..6   (lanes 7..15 idle)
//     slot 1: rows  7 .. 22 in lanes 0..15
//     slot 2: rows 23 .. 38 in lanes 0..15
// Row / column k of the matrices lives in lane quad_lane_of(k) of slot quad_slot(k) of
// every DPP row, so one row_newbcast DPP operand reaches the element of all four matrices
// at once -- no v_readlane, no SGPR round trip, no LDS.  The elimination the kernels use
// works on the lower triangle only (spkd_tri.hpp): slot s then needs the columns below
// its last row, and column J costs one FMA per slot that holds a row >= J.  Filling the
// LATE slots to all 16 lanes is what keeps both small: 7 + 23 + 39 = 69 doubles per lane
// and 1 015 FMAs per elimination, the least 16-lane rows allow (the even split 13/13/13
// takes 78 and 1 144).  The full-square and column-blocked forms the triangular one
// superseded live in tools/ with the micro-benchmarks that compare them.
//
// The split is stated ONCE, as the slot bases below; every index in the library that
// depends on it is derived from them here.
#pragma once
#include "spkd_device.hpp"

namespace spkd {

constexpr int QS = 3;         // row slots per lane

// first row of each slot (A/B builds: make variant FLAGS=-DSPKD_QUAD_BASES=0,13,26)
#ifndef SPKD_QUAD_BASES
#define SPKD_QUAD_BASES 0, 7, 23
#endif
__host__ __device__ constexpr int quad_base_pick(int s, int b0, int b1, int b2) {
    return s <= 0 ? b0 : (s == 1 ? b1 : (s == 2 ? b2 : D));
}
__host__ __device__ constexpr int quad_base(int s) { return quad_base_pick(s, SPKD_QUAD_BASES); }    // s = QS: D
__host__ __device__ constexpr int quad_rows(int s) { return quad_base(s + 1) - quad_base(s); }      // rows of slot s
__host__ __device__ constexpr int quad_row(int s, int t) { return quad_base(s) + t; }               // t < quad_rows(s)
__host__ __device__ constexpr int quad_slot(int r) { return r >= quad_base(2) ? 2 : (r >= quad_base(1) ? 1 : 0); }
__host__ __device__ constexpr int quad_lane_of(int r) { return r - quad_base(quad_slot(r)); }
// columns of the lower triangle held by slot s: 0 .. tri_cols(s) - 1
__host__ __device__ constexpr int tri_cols(int s) { return quad_base(s + 1); }

// lanes of a DPP row that carry a row in some slot
constexpr int QLANES = quad_rows(0) > quad_rows(1) ? (quad_rows(0) > quad_rows(2) ? quad_rows(0) : quad_rows(2))
                                                   : (quad_rows(1) > quad_rows(2) ? quad_rows(1) : quad_rows(2));
static_assert(quad_base(0) == 0 && quad_rows(0) > 0 && quad_rows(1) > 0 && quad_rows(2) > 0 && QLANES <= 16, "slot bases");
static_assert(quad_rows(0) < 16, "lane 15 of slot 0 holds the frame count");

// Loads from a PACKED record (the ABI format).  Read by symmetry it is the lower triangle
// column by column (column j holds rows j .. 39 contiguously from pk_off(j)), so the load of
// (slot s, column j) is consecutive doubles at quad_pk_at(s, j) + t.  Lanes of a diagonal
// block above the diagonal land in the previous column's tail, and the idle lanes of a
// short slot read on into the column: both inside the record, into registers that are
// never a DPP source and never stored.  Lanes past QLANES (none with the default split)
// ride with the last one.  The sums entry of this lane's row c is pk_off(c) + D - c.
__host__ __device__ constexpr int quad_pk_at(int s, int j) { return pk_off(j) + quad_base(s) - j; }
__device__ __forceinline__ int quad_load_lane(int t) {
    if constexpr (QLANES < 16) return t < QLANES ? t : QLANES - 1;
    else return t;
}
constexpr bool quad_loads_in_record() {
    for (int s = 0; s < QS; ++s) {
        if (quad_base(s) + QLANES - 1 >= D) return false;                      // sums: a row of the matrix
        for (int j = 0; j < tri_cols(s); ++j)
            if (quad_pk_at(s, j) < 0 || quad_pk_at(s, j) + QLANES - 1 >= REC) return false;
    }
    return true;
}
static_assert(quad_loads_in_record(), "a packed load of some (slot, column, lane) leaves the record");

struct QuadRows {
    double r[QS][D];
};

// broadcast lane K (0..15) of every 16-lane row to the whole row
template <int K>
__device__ __forceinline__ double bcast16(double v) {
    const long long x = __double_as_longlong(v);
    return __longlong_as_double(__builtin_amdgcn_update_dpp(0ll, x, 0x150 + K, 0xf, 0xf, true));
}

// 1 / x to ~1 ulp: hardware estimate + two Newton steps (5 instructions instead of the
// ~15 of an IEEE division; the multipliers are not part of any parity contract)
__device__ __forceinline__ double fast_recip(double x) {
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}

}  // namespace spkd

// ===========================================================================
// Quad records: the storage format the clustering kernels keep their working set
// in.  QREC = 3 slots x 40 columns x 16 lanes doubles (15 360 B):
//     qr[(s * 40 + j) * 16 + t] = M(quad_row(s, t), j)   for t < quad_rows(s) (M = augmented moments)
// so that a wave's load of (slot s, column j) is one 128-B line per DPP row --
// perfectly coalesced for the quad row layout.  Column 39 holds the sums; the frame
// count sits in lane 15 of (slot 0, column 39), which carries no row.
// Records add component-wise (padding stays zero).
// ===========================================================================
namespace spkd {

constexpr int QREC = QS * DA * 16;
constexpr int QREC_COUNT_AT = (0 * DA + D) * 16 + 15;

__host__ __device__ constexpr int qr_index(int i, int j) { return (quad_slot(i) * DA + j) * 16 + quad_lane_of(i); }

struct QuadLane {
    int m;       // matrix index inside the wave (DPP row), 0..3
    int t;       // lane inside the DPP row, 0..15
};

__device__ __forceinline__ QuadLane quad_lane() {
    QuadLane L;
    const int lane = lane_id();
    L.m = lane >> 4;
    L.t = lane & 15;
    return L;
}

__device__ __forceinline__ double qr_count(const double* __restrict__ qr) { return qr[QREC_COUNT_AT]; }

// q = w * record rows (global or LDS pointer); sv[s] = sums column
__device__ __forceinline__ void quad_load_scaled(const double* __restrict__ qr, int t, double w,
                                                 QuadRows& q, double (&sv)[QS]) {
#pragma unroll
    for (int s = 0; s < QS; ++s) {
#pragma unroll
        for (int j = 0; j < D; ++j) q.r[s][j] = w * qr[(s * DA + j) * 16 + t];
        sv[s] = qr[(s * DA + D) * 16 + t];
    }
}


// ===========================================================================
// Tri records: the quad lane layout restricted to what the symmetric elimination reads,
// in 128-byte lines: line (tri_off(s) + j) holds M(quad_row(s, t), j) for t < quad_rows(s),
// j < tri_cols(s); the QS lines from TREC_SUMS hold the sums column of slot s; the frame
// count sits in lane 15 of the first of them (slot 0 leaves it free).  7 + 23 + 39 + 3 =
// 72 lines = 9 216 B; every load of (slot s, column j) is one aligned line per DPP row.
// ===========================================================================
__host__ __device__ constexpr int tri_off(int s) {           // lines before slot s (s = QS: all)
    return s <= 0 ? 0 : (s == 1 ? tri_cols(0) : (s == 2 ? tri_cols(0) + tri_cols(1) : tri_cols(0) + tri_cols(1) + tri_cols(2)));
}
constexpr int TREC_SUMS = tri_off(QS);                       // first sums line (69)
constexpr int TLINES = TREC_SUMS + QS;                       // 72
constexpr int TREC = TLINES * 16;                            // 1 152 doubles = 9 216 B
constexpr int TREC_COUNT_AT = TREC_SUMS * 16 + 15;

// entry (row r, column j <= r) of the 40x40 augmented matrix -> index in a tri record:
// 16 j + r + a constant of r's slot (one select chain for a run-time r)
__host__ __device__ constexpr int tri_row_at(int r) {          // (row r < D, column 0)
    return r + (r >= quad_base(2) ? tri_off(2) * 16 - quad_base(2) : (r >= quad_base(1) ? tri_off(1) * 16 - quad_base(1) : 0));
}
__host__ __device__ constexpr int tri_sum_at(int j) {          // (row D, column j < D)
    return TREC_SUMS * 16 + j + (j >= quad_base(2) ? 32 - quad_base(2) : (j >= quad_base(1) ? 16 - quad_base(1) : 0));
}
__device__ __forceinline__ int tri_slot(int r, int j) {
    if (r < D) return tri_row_at(r) + 16 * j;
    if (j < D) return tri_sum_at(j);
    return TREC_COUNT_AT;
}
static_assert(tri_row_at(quad_row(1, 2)) == (tri_off(1) * 16 + 2) && tri_row_at(quad_row(2, 15 < quad_rows(2) ? 15 : 0)) == tri_off(2) * 16 + (15 < quad_rows(2) ? 15 : 0)
              && tri_sum_at(quad_row(2, 1)) == (TREC_SUMS + 2) * 16 + 1, "tri record index");


// tri-record index idx -> packed index holding the same entry (-1: padding)
__device__ __forceinline__ int tri_image_source(int idx) {
    const int t = idx & 15, line = idx >> 4;
    if (line >= TREC_SUMS) {                     // sums lines: (39, row of (s, t)), the count in lane 15 of the first
        const int s = line - TREC_SUMS;
        if (t < quad_rows(s)) return pk_low(D, quad_row(s, t));
        return idx == TREC_COUNT_AT ? REC - 1 : -1;
    }
    const int s = line < tri_off(1) ? 0 : (line < tri_off(2) ? 1 : 2);
    if (t >= quad_rows(s)) return -1;
    const int j = line - tri_off(s);
    const int r = quad_row(s, t);
    return r >= j ? pk_low(r, j) : pk_low(j, r);
}


}  // namespace spkd
