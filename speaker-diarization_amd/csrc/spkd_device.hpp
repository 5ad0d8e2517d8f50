// Wave-level (64-lane) building blocks shared by every kernel in this library.
//
// Layout convention ("row layout"): lane i (0..38) owns row i of a 39x39 matrix
// in 39 doubles held in registers; lane 39 owns the augmented row (sums, count);
// lanes 40..63 ride along with row 39's values and are ignored.  All loops over
// columns are fully unrolled so register indices are static; cross-lane data
// moves with v_readlane (static or wave-uniform source lane) -- no LDS.
//
// gfx950 only: wave64, no MFMA (the statistics are O(d^2) per frame and the
// factorisation is a 39-step dependent chain; throughput comes from many
// independent matrices in flight).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spkd {

constexpr int D = 39;          // feature dimension
constexpr int DA = 40;         // augmented dimension ([x; 1])
constexpr int REC = 820;       // packed upper triangle of DA x DA
constexpr int WAVE = 64;
// pointer to global memory in a non-kernel function: a plain pointer there is generic,
// its loads and stores are flat_* and count in lgkmcnt too, so every LDS wait would also
// wait for the global loads and stores in flight
#define SPKD_GLOBAL __attribute__((address_space(1)))
constexpr int REC_PER_LANE = 13;   // ceil(820 / 64)

__host__ __device__ constexpr int pk_off(int r) { return r * DA - (r * (r - 1)) / 2; }
__host__ __device__ constexpr int pk(int r, int c) { return pk_off(r) + (c - r); }   // r <= c

// entry (row r, column j <= r) of the lower triangle in a packed record: by symmetry
// pk(j, r), so column j holds its rows j .. 39 contiguously from pk_off(j)
__host__ __device__ constexpr int pk_low(int r, int j) { return pk_off(j) + (r - j); }

__device__ __forceinline__ void decode_entry(int e, int& r, int& c) {
    int rr = 0;
#pragma unroll 1
    while (rr + 1 < DA && pk_off(rr + 1) <= e) ++rr;
    r = rr;
    c = rr + (e - pk_off(rr));
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

__device__ __forceinline__ double readlane_d(double v, int src_lane) {
    // src_lane must be wave-uniform
    int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ long long uniform_ll(long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

template <class T>
__device__ __forceinline__ T* uniform_p(T* p) { return (T*)uniform_ll((long long)p); }

__device__ __forceinline__ double uniform_d(double v) {
    int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// ---------------------------------------------------------------------------
// Packed record -> row layout through a per-wave LDS slab of REC doubles.
//
// stage(): coalesced copy (13 doubles per lane) of  g1 [+ sgn * g2]  into the slab.
// row_from_slab(): q[j] = M(lane, j) for j = 0..39 (q[39] = sum of x_lane;
// lane 39 gets the sums row, its q[39] is the frame count).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void stage1(double* slab, const double* __restrict__ g) {
    const int lane = lane_id();
#pragma unroll
    for (int m = 0; m < REC_PER_LANE; ++m) {
        int e = lane + WAVE * m;
        if (e < REC) slab[e] = g[e];
    }
}

__device__ __forceinline__ void stage2(double* slab, const double* __restrict__ g1,
                                       const double* __restrict__ g2, double sgn) {
    const int lane = lane_id();
#pragma unroll
    for (int m = 0; m < REC_PER_LANE; ++m) {
        int e = lane + WAVE * m;
        if (e < REC) slab[e] = g1[e] + sgn * g2[e];
    }
}

__device__ __forceinline__ void row_from_slab(const double* slab, double (&q)[DA]) {
    int i = lane_id();
    i = i > D ? D : i;
    const int base_i = pk_off(i) - i;
#pragma unroll
    for (int j = 0; j < DA; ++j) {
        const int cj = pk_off(j) - j;
        int idx = (i <= j) ? (base_i + j) : (cj + i);
        q[j] = slab[idx];
    }
}

// q[j] += sgn * M(lane, j) from a slab
__device__ __forceinline__ void row_acc_slab(const double* slab, double (&q)[DA], double sgn) {
    int i = lane_id();
    i = i > D ? D : i;
    const int base_i = pk_off(i) - i;
#pragma unroll
    for (int j = 0; j < DA; ++j) {
        const int cj = pk_off(j) - j;
        int idx = (i <= j) ? (base_i + j) : (cj + i);
        q[j] = fma(sgn, slab[idx], q[j]);
    }
}

// Expanded LDS image of one record: ex[j * DA + i] = M(i, j), i, j in 0..39.
// Conflict-free for row-layout reads (consecutive lanes -> consecutive doubles).
__device__ __forceinline__ void expand_to_lds(double* ex, const double* __restrict__ g,
                                              int tid, int nthreads) {
    for (int t = tid; t < DA * DA; t += nthreads) {
        int j = t / DA, i = t - j * DA;
        int r = i < j ? i : j, c = i < j ? j : i;
        ex[t] = g[pk(r, c)];
    }
}

__device__ __forceinline__ void row_from_expanded(const double* ex, double (&q)[DA]) {
    int i = lane_id();
    i = i > D ? D : i;
#pragma unroll
    for (int j = 0; j < DA; ++j) q[j] = ex[j * DA + i];
}

// ---------------------------------------------------------------------------
// Covariance rows from second-moment rows:  np.cov(x, rowvar=0) semantics
// (numpy: subtract the mean, X^T X, multiply by 1/(n-1)) restated on raw
// moments: S_ij = (Q_ij - s_i s_j / n) * (1/(n-1)).
// q: second-moment row (q[39] = s_lane), overwritten by the covariance row;
// n = frame count (uniform).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void cov_rows(double (&q)[DA], double n) {   // in place
    const double inv_n = 1.0 / n;
    const double f = 1.0 / (n - 1.0);
    const double mi = -(q[D] * inv_n);
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double sj = readlane_d(q[D], j);
        q[j] = fma(mi, sj, q[j]) * f;
    }
}

// true when every entry of every real row (lanes 0..38) is finite
__device__ __forceinline__ bool rows_finite(const double (&a)[DA]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < D; ++j) ok = ok && (fabs(a[j]) < __builtin_huge_val());
    ok = ok || (lane_id() >= D);
    return __all(ok);
}

// ---------------------------------------------------------------------------
// Determinant by Gaussian elimination, row layout.
//
// det_nopivot: for the symmetric positive definite case (every covariance of
// >= 40 real frames).  Straight-line code: 741 fp64 FMAs, pivot rows broadcast
// with static-lane v_readlane.  Returns false if some pivot is not a positive
// finite number; the caller then re-forms the matrix and calls det_pivoted.
//
// det_pivoted: partial pivoting with LAPACK dgetf2 semantics (first maximum in
// current row order, zero pivot => that elimination step is skipped), product
// of pivots in order k = 0..38 times the permutation sign -- the quantity
// scipy.linalg.det returns (scipy/linalg/_basic.py det -> getrf + diagonal
// product).  Destroys a.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool det_nopivot(double (&a)[DA], double& det_out) {
    double det = 1.0;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double piv = readlane_d(a[k], k);
        ok = ok && (piv > 0.0) && (piv < __builtin_huge_val());
        det *= piv;
        const double l = -(a[k] * (1.0 / piv));
#pragma unroll
        for (int j = k + 1; j < D; ++j) {
            const double u = readlane_d(a[j], k);
            a[j] = fma(l, u, a[j]);
        }
    }
    det_out = det;
    return ok;
}

__device__ __forceinline__ double det_pivoted(double (&a)[DA]) {
    const int lane = lane_id();
    int pos = lane;                       // current position of this row
    double det = 1.0;
    bool neg = false;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        // arg max |a[k]| over rows at positions >= k; ties -> smallest position
        double v = (lane < D && pos >= k) ? fabs(a[k]) : -1.0;
        if (v != v) v = -0.5;             // NaNs never win (idamax compares with >)
        int p = pos;
        int src = lane;
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) {
            double v2 = __shfl_xor(v, m);
            int p2 = __shfl_xor(p, m);
            int s2 = __shfl_xor(src, m);
            bool take = (v2 > v) || (v2 == v && p2 < p);
            v = take ? v2 : v;
            p = take ? p2 : p;
            src = take ? s2 : src;
        }
        const int ps = uniform_i(src);    // lane holding the pivot row
        const int pp = uniform_i(p);      // its position
        const double piv = readlane_d(a[k], ps);
        if (pp != k) {                    // row interchange
            neg = !neg;
            int newpos = pos;
            if (pos == k) newpos = pp;
            if (lane == ps) newpos = k;
            pos = newpos;
        }
        det *= piv;
        double l = 0.0;
        if (piv != 0.0 && pos > k && lane < D) l = -(a[k] * (1.0 / piv));
#pragma unroll
        for (int j = k + 1; j < D; ++j) {
            const double u = readlane_d(a[j], ps);
            a[j] = fma(l, u, a[j]);
        }
    }
    return neg ? -det : det;
}

// In-place inverse of a symmetric positive definite matrix (Gauss-Jordan without
// pivoting, row layout); returns false when a pivot is not positive finite.
// Used for the diagonal of pinv(S) in KL2 (full rank: pinv == inverse).
__device__ __forceinline__ bool invert_spd(double (&a)[DA]) {
    const int lane = lane_id();
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double piv = readlane_d(a[k], k);
        ok = ok && (piv > 0.0) && (piv < __builtin_huge_val());
        const double r = 1.0 / piv;
        const double aik = a[k];
        const bool isk = (lane == k);
        const double l = isk ? 0.0 : -(aik * r);
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j == k) continue;
            const double u = readlane_d(a[j], k);
            a[j] = isk ? u * r : fma(l, u, a[j]);
        }
        a[k] = isk ? r : l;               // column k of the inverse-in-progress
    }
    return ok;
}

// a[lane] without dynamic register indexing
__device__ __forceinline__ double diag_of(const double (&a)[DA]) {
    const int lane = lane_id();
    double v = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) v = (lane == j) ? a[j] : v;
    return v;
}

__device__ __forceinline__ double wave_sum39(double v) {
    v = (lane_id() < D) ? v : 0.0;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// ---------------------------------------------------------------------------
// log(det(A)) of a matrix produced by `form(a)` (fills a[0..38] per lane).
// Non-finite entries: the reference's scipy.linalg.det raises ValueError
// ("array must not contain infs or NaNs"); here the error bit is raised and
// NaN returned.  Fast path = det_nopivot; if that meets a non-positive pivot the
// matrix is formed again and eliminated with partial pivoting.
// numpy.log semantics: log(0) = -inf, log(negative) = NaN.
// ---------------------------------------------------------------------------
constexpr int ERR_NONFINITE = 1;

// Out-of-line slow paths.  The straight-line eliminations are several thousand
// instructions each; inlining the rarely taken ones at every call site blows the
// kernels far past the instruction cache (k_gw was > 500 KB of code), so they are
// real functions, emitted once per code object, taking the row array by pointer.
// determinant by partial pivoting (NaN + the error bit for non-finite input); its log,
// taken by the caller, is what scipy.linalg.det + numpy.log give: 0 -> -inf, negative -> NaN
__device__ __noinline__ double det_pivoted_fn(const double* rows, int* err) {
    double a[DA];
#pragma unroll
    for (int j = 0; j < DA; ++j) a[j] = rows[j];
    if (!rows_finite(a)) {
        if (lane_id() == 0) atomicOr(err, ERR_NONFINITE);
        return __builtin_nan("");
    }
    return det_pivoted(a);
}

__device__ __forceinline__ double logdet_pivoted_fn(const double* rows, int* err) {
    return log(det_pivoted_fn(rows, err));
}

template <class Form>
__device__ __forceinline__ double logdet_formed(double (&a)[DA], int* err, Form form) {
    form(a);
    if (!rows_finite(a)) {
        if (lane_id() == 0) atomicOr(err, ERR_NONFINITE);
        return __builtin_nan("");
    }
    double det;
    if (!det_nopivot(a, det)) {
        form(a);
        return logdet_pivoted_fn(a, err);
    }
    return log(det);
}

// ---------------------------------------------------------------------------
// diag(pinv(S)) of a symmetric 39x39 covariance, scipy.linalg.pinv semantics (the
// reference's kl2, spk-clustering.py:124-133): eigenvalues |lambda| > 39 eps max|lambda|
// are kept (strictly, so S = 0 gives 0), diag_i = sum over kept k of V_ik^2 / lambda_k.
//
// Parallel (round-robin) Jacobi, one wave: step t of a sweep rotates the 20 disjoint pairs
// (t, 39) and ((t + k) mod 39, (t - k) mod 39), k = 1..19 -- index 39 is a zero dummy, so
// every pair (p, q) of 0..38 is met once per 39 steps.  A step updates A <- J^T A J and
// V <- V J as 20 x 20 independent 2 x 2 blocks, each read and written by one lane, so the
// only ordering a step needs is against the step before.  A and V (2 x 40 x 40 doubles)
// live in a slab of the context's device workspace: the calling kernels keep their LDS.
//
// Workspace: PINV_LOCK_BYTES of lock words, then PINV_XCC x PINV_SLABS_PER_XCC slabs.  A
// wave takes a free slab of its own XCD's pool (L2s of different XCDs are not coherent
// inside one launch; a slab never changes XCD within a launch) and writes every cell it
// will read before reading it, so nothing a previous holder left behind is ever seen.
// More waves in the fallback on one XCD than it has slabs wait for one (s_sleep between
// attempts); a holder waits for nothing, so every waiter gets one.
// ---------------------------------------------------------------------------
constexpr int PINV_XCC = 8;
constexpr int PINV_SLABS_PER_XCC = 128;
constexpr int PINV_SLAB = 2 * DA * DA;                 // doubles: A | V
constexpr size_t PINV_LOCK_BYTES = (size_t)PINV_XCC * PINV_SLABS_PER_XCC * sizeof(unsigned);
constexpr size_t PINV_WS_BYTES =
    PINV_LOCK_BYTES + (size_t)PINV_XCC * PINV_SLABS_PER_XCC * PINV_SLAB * sizeof(double);
constexpr int PINV_MAX_SWEEPS = 40;                    // not converged by then: NaN
constexpr int PINV_PAIRS = DA / 2;                     // rotations per step
constexpr int PINV_BLOCKS = PINV_PAIRS * PINV_PAIRS;   // 2 x 2 blocks per step
// Fast path: invert_spd succeeded and tr(S) tr(S^-1) <= PINV_FAST_BOUND implies
// lambda_min / lambda_max > 39 eps (lambda_max <= tr S, lambda_min >= 1 / tr S^-1): every
// eigenvalue is kept, pinv == inverse.  1e-3 / (39 eps).
constexpr double PINV_FAST_BOUND = 1e-3 / (39.0 * 2.220446049250313e-16);

// pair k of step t, p < q (pair 0: (t, 39), the identity)
__device__ __forceinline__ void pinv_pair(int t, int k, int& p, int& q) {
    int a = t + k, b = t - k;
    a = a >= D ? a - D : a;
    b = b < 0 ? b + D : b;
    p = k == 0 ? t : (a < b ? a : b);
    q = k == 0 ? D : (a < b ? b : a);
}

__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// orders the slab accesses of one step against the next (lanes of one wave read what
// other lanes wrote): no code motion across it, and the stores have completed
__device__ __forceinline__ void pinv_step_fence() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_s_waitcnt(0);
}

__device__ __noinline__ double pinv_diag_fn(const double* rows, double* ws) {
    const int lane = lane_id();
    double a[DA];
#pragma unroll
    for (int j = 0; j < DA; ++j) a[j] = rows[j];
    if (!rows_finite(a)) return __builtin_nan("");   // (the reference's pinv raises; the caller flags it)
    // a free slab of this XCD's pool (HW_REG_XCC_ID: hwreg id 20, bits [3:0])
    unsigned* locks = (unsigned*)ws;
    const int xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11)) & (PINV_XCC - 1);
    int slot = 0;
    if (lane == 0) {
        int i = (int)((blockIdx.x + blockIdx.y * 7u + (threadIdx.x >> 6) * 13u) % PINV_SLABS_PER_XCC);
        unsigned* pool = locks + xcc * PINV_SLABS_PER_XCC;
        while (atomicCAS(pool + i, 0u, 1u) != 0u) {
            i = i + 1 == PINV_SLABS_PER_XCC ? 0 : i + 1;
            if (i == 0) __builtin_amdgcn_s_sleep(8);
        }
        slot = xcc * PINV_SLABS_PER_XCC + i;
    }
    slot = __builtin_amdgcn_readfirstlane(__shfl(slot, 0));
    double* A = (double*)((char*)ws + PINV_LOCK_BYTES) + (size_t)slot * PINV_SLAB;
    double* V = A + DA * DA;
    // A = S with a zero row / column 39, V = I (both symmetric: lane i writes column i,
    // consecutive lanes consecutive doubles)
    double fro = 0.0;
    if (lane < DA) {
#pragma unroll
        for (int j = 0; j < DA; ++j) {
            const double v = (lane < D && j < D) ? a[j] : 0.0;
            fro = fma(v, v, fro);
            A[j * DA + lane] = v;
            V[j * DA + lane] = lane == j ? 1.0 : 0.0;
        }
    }
    // a pair is rotated when |a_pq| > max(1e-15 sqrt|a_pp a_qq|, 1e-15 ||S||_F): the second
    // term is the rounding floor (the rotations keep regenerating off-diagonal noise of
    // ~eps ||S|| between the kept and the cut eigenvectors of a singular S); converged = a
    // sweep without a rotation
    const double floor_abs = 1e-15 * sqrt(wave_sum64(fro));
    bool conv = false;
#pragma unroll 1
    for (int sweep = 0; sweep < PINV_MAX_SWEEPS && !conv; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int t = 0; t < D; ++t) {
            // lane k < 20: the rotation of pair k (numerical-recipes form, as oracle/spkd_oracle.c)
            double cr = 1.0, sr = 0.0;
            bool rot = false;
            if (lane > 0 && lane < PINV_PAIRS) {
                int p, q;
                pinv_pair(t, lane, p, q);
                const double apq = A[p * DA + q];
                const double app = A[p * DA + p], aqq = A[q * DA + q];
                rot = fabs(apq) > fmax(1e-15 * sqrt(fabs(app * aqq)), floor_abs);
                if (rot) {
                    const double th = (aqq - app) / (2.0 * apq);
                    // (|theta| > 1e150: theta^2 would overflow, t = 1 / (2 theta) to working precision)
                    const double tt = fabs(th) > 1e150 ? 0.5 / th
                                    : (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                    cr = 1.0 / sqrt(tt * tt + 1.0);
                    sr = tt * cr;
                }
            }
            if (!__any(rot)) continue;                 // (uniform)
            rotated = true;
#pragma unroll
            for (int it = 0; it < (PINV_BLOCKS + WAVE - 1) / WAVE; ++it) {
                const int b = lane + WAVE * it;
                const bool on = b < PINV_BLOCKS;
                const int P = on ? b / PINV_PAIRS : 0, Q = on ? b - (b / PINV_PAIRS) * PINV_PAIRS : 0;
                const double cP = __shfl(cr, P), sP = __shfl(sr, P);
                const double cQ = __shfl(cr, Q), sQ = __shfl(sr, Q);
                if (on) {
                    int p, q, r, s;
                    pinv_pair(t, P, p, q);
                    pinv_pair(t, Q, r, s);
                    const double apr = A[p * DA + r], aps = A[p * DA + s];
                    const double aqr = A[q * DA + r], aqs = A[q * DA + s];
                    const double vpr = V[p * DA + r], vps = V[p * DA + s];
                    const double vqr = V[q * DA + r], vqs = V[q * DA + s];
                    // columns (r, s) by J_Q, then rows (p, q) by J_P^T
                    const double xpr = cQ * apr - sQ * aps, xps = sQ * apr + cQ * aps;
                    const double xqr = cQ * aqr - sQ * aqs, xqs = sQ * aqr + cQ * aqs;
                    A[p * DA + r] = cP * xpr - sP * xqr;
                    A[q * DA + r] = sP * xpr + cP * xqr;
                    A[p * DA + s] = cP * xps - sP * xqs;
                    A[q * DA + s] = sP * xps + cP * xqs;
                    V[p * DA + r] = cQ * vpr - sQ * vps;
                    V[p * DA + s] = sQ * vpr + cQ * vps;
                    V[q * DA + r] = cQ * vqr - sQ * vqs;
                    V[q * DA + s] = sQ * vqr + cQ * vqs;
                }
            }
            pinv_step_fence();
        }
        conv = !rotated;
    }
    // eigenvalues on the diagonal; the cut-off; lane i < 39: sum_k V_ik^2 / lambda_k
    const int li = lane < D ? lane : 0;
    const double lam = A[li * DA + li];
    double lmax = lane < D ? fabs(lam) : 0.0;
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) lmax = fmax(lmax, __shfl_xor(lmax, m));
    const double cut = 39.0 * 2.220446049250313e-16 * lmax;
    double acc = 0.0;
#pragma unroll 1
    for (int k = 0; k < D; ++k) {
        const double lk = readlane_d(lam, k);
        const double v = V[li * DA + k];
        if (fabs(lk) > cut) acc += v * v / lk;
    }
    pinv_step_fence();
    if (lane == 0) atomicExch(locks + slot, 0u);
    return conv ? acc : __builtin_nan("");
}

// out[0] = S_ii, out[1] = (S^-1)_ii (NaN if S is not positive definite), for the
// lane's row of the covariance held in rows[] (row-per-lane layout).  pinv_ws != nullptr:
// out[1] = pinv(S)_ii instead -- the inverse's when the fast-path bound holds, else
// pinv_diag_fn's.
__device__ __noinline__ void spd_diag_terms_fn(const double* rows, double* out, double* pinv_ws) {
    double a[DA];
#pragma unroll
    for (int j = 0; j < DA; ++j) a[j] = rows[j];
    const double ds = diag_of(a);
    out[0] = ds;
    const bool ok = invert_spd(a);
    double dp = diag_of(a);
    if (!ok) dp = __builtin_nan("");
    if (pinv_ws) {
        const double tr = wave_sum39(ds) * wave_sum39(dp);   // (NaN when !ok)
        if (!(ok && tr <= PINV_FAST_BOUND)) dp = pinv_diag_fn(rows, pinv_ws);
    }
    out[1] = dp;
}

}  // namespace spkd
